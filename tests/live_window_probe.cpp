// Host build of uhc_amd/csrc/uhc_live_window.h for tests/test_live_window_cpu.py: the window rule uhc_live.hip's slide kernel calls, and the move it makes,
// as plain loops.  No HIP header, no hipcc.  With -DLIVE_WINDOW_PROBE_MAIN the file is a program of its own (for a run under the host sanitizers).
#include "uhc_live_window.h"

#define PROBE_API extern "C" __attribute__((visibility("default")))

// S for n cases at once: in [n][4] = (len, cap, start_ind, cur_t)
PROBE_API void uhc_live_window_probe_discard(int n, const int* in, int* out) {
    for (int i = 0; i < n; i++) out[i] = uhc_lw_discard(in[4 * i], in[4 * i + 1], in[4 * i + 2], in[4 * i + 3]);
}

// The slide of one env as the kernel makes it, one "lane" after the other: slice [cap][width], state = (len, start_ind, base, moved), in and out.  Every lane
// moves its own columns of every record in ascending record order; the lanes run one after the other here, the extreme of every interleaving.
// Returns S.
PROBE_API int uhc_live_window_probe_slide(int cap, int width, int lanes, double* slice, int cur_t, int* state) {
    int len = state[0] < 0 ? 0 : (state[0] > cap ? cap : state[0]);
    int S = uhc_lw_discard(len, cap, state[1], cur_t);
    S = S < 0 ? 0 : S;
    S = S > len - 1 ? len - 1 : S;
    if (S < 1) return 0;
    for (int lane = 0; lane < lanes; lane++)
        for (int k = S; k < len; k++)
            for (int j = lane; j < width; j += lanes) slice[(long)(k - S) * width + j] = slice[(long)k * width + j];
    state[0] = len - S, state[1] -= S, state[2] += S, state[3] += len - S;
    return S;
}

#ifdef LIVE_WINDOW_PROBE_MAIN
#include <stdio.h>
#include <stdlib.h>
int main() {
    long cases = 0;
    for (int cap = 1; cap <= 8; cap++)
        for (int len = 0; len <= cap; len++)
            for (int si = -8; si <= 8; si++)
                for (int t = 0; t <= 16; t++) {
                    if (si + t < 0) continue;
                    int in[4] = {len, cap, si, t}, S;
                    uhc_live_window_probe_discard(1, in, &S);
                    if (S < 0 || (len > 0 && S > len - 1) || S > si + t || (len < cap && S != 0)) return printf("rule: %d %d %d %d -> %d\n", len, cap, si, t, S), 1;
                    double* slice = (double*)malloc(sizeof(double) * cap * 7);  // exactly the slice: the sanitizer sees any index beyond it
                    for (int i = 0; i < cap * 7; i++) slice[i] = i / 7;
                    int st[4] = {len, si, 0, 0};
                    const int got = uhc_live_window_probe_slide(cap, 7, 3, slice, t, st);
                    if (got != S) return printf("slide: %d != %d\n", got, S), 1;
                    for (int k = 0; k < st[0] && got; k++)
                        for (int j = 0; j < 7; j++)
                            if (slice[k * 7 + j] != k + S) return printf("move: %d %d %d %d slot %d\n", len, cap, si, t, k), 1;
                    free(slice);
                    cases++;
                }
    printf("live_window_probe: %ld cases ok\n", cases);
    return 0;
}
#endif
