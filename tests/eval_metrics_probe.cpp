// eval_metrics_probe.cpp -- thin C interface over uhc_amd/csrc/uhc_eval_metrics.h for tests/test_eval_metrics_cpu.py: built with the host compiler, no HIP.
// The header's pieces are what the device kernel (uhc_eval.hip) computes a row with; here the sums over the joints are the header's own serial loops.
#include "uhc_eval_metrics.h"

#define PROBE_API extern "C" __attribute__((visibility("default")))

// every row of one clip: pred_q [T][nqh], gt_q [T][ngq] (7 numbers of a row are read), pj / gj [T][72]; out [T][6], untouched where numpy's arrays are shorter
PROBE_API void uhc_eval_probe_clip(const double* pred_q, int nqh, const double* gt_q, int ngq, const double* pj, const double* gj, int T, double* out) {
    for (int t = 0; t < T; t++) {
        const int n_next = T - 1 - t < 2 ? T - 1 - t : 2;
        const double* const p3[3] = {pj + 72 * t, pj + 72 * (t + (n_next >= 1 ? 1 : 0)), pj + 72 * (t + (n_next >= 2 ? 2 : 0))};
        const double* const g3[3] = {gj + 72 * t, gj + 72 * (t + (n_next >= 1 ? 1 : 0)), gj + 72 * (t + (n_next >= 2 ? 2 : 0))};
        uhc_em_row_serial(pred_q + (long)nqh * t, gt_q + (long)ngq * t, p3, g3, n_next, T, out + UHC_EM_NMETRIC * t);
    }
}

// H [9] row-major -> U [9], s [3], V [9] (vectors in columns)
PROBE_API void uhc_eval_probe_svd3(const double* H, double* U, double* s, double* V) {
    double h[9], u[9], sv[3], v[9];
    for (int i = 0; i < 9; i++) h[i] = H[i];
    uhc_em_svd3(h, u, sv, v);
    for (int i = 0; i < 9; i++) U[i] = u[i], V[i] = v[i];
    for (int i = 0; i < 3; i++) s[i] = sv[i];
}
