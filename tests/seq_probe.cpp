// Host build of uhc_amd/csrc/uhc_seq.h for tests/test_seq_cpu.py: the sequence rules the post-processing kernels share, each behind one extern "C" wrapper.
// No HIP header, no hipcc.
#include "uhc_seq.h"

#define PROBE_API extern "C" __attribute__((visibility("default")))

PROBE_API int uhc_seq_probe_rows(int r, int row_cap) { return uhc_seq_rows(r, row_cap); }
PROBE_API long long uhc_seq_probe_start(long long g, int T, long long n_rows_total) { return uhc_seq_start(g, T, n_rows_total); }
PROBE_API int uhc_seq_probe_model(const int* model, long long s, int n_models) { return uhc_seq_model(model, s, n_models); }
PROBE_API int uhc_seq_probe_clip(const int* clip_start, int n_clips, long long f) { return uhc_clip_of(clip_start, n_clips, f); }
PROBE_API int uhc_seq_probe_packed_byte(const unsigned long long* w3, int i) {
    const unsigned long long w[3] = {w3[0], w3[1], w3[2]};
    return uhc_packed_byte(w, i);
}
PROBE_API double uhc_seq_probe_nan() { return uhc_nan(); }
PROBE_API double uhc_seq_probe_mean(const double* rows, int stride, int k, long long g0, int n) { return uhc_seq_mean(rows, stride, k, g0, n); }
