// CPU probe over uhc_amd/csrc/uhc_policy_math.h (tests/test_policy_pack_cpu.py): the index maps of the packed weight and the packed activation, a host
// emulation of uhc_policy_layer_kernel built from the same lane maps -- operands gathered lane by lane, the 16 x 16 x 4 product formed as the instruction
// defines it, the result stored through the C / D -> next-A map --, the activations and the filter's rule.  (The kernel also splits K over its four waves and
// adds the runs in wave order; on the integer data of the tests every order gives the same bits, so the emulation walks K in one run.)
#include <stdint.h>

#include <vector>

#include "uhc_policy_math.h"

#define EXPORT extern "C" __attribute__((visibility("default")))

EXPORT int64_t pol_w_index(int n, int k, int kpad) { return (int64_t)uhc_pol_w_index(n, k, kpad); }
EXPORT int64_t pol_x_index(int r, int k, int kpad) { return (int64_t)uhc_pol_x_index(r, k, kpad); }
EXPORT int64_t pol_w_doubles(int out, int in) { return (int64_t)uhc_pol_w_doubles(out, in); }
EXPORT int64_t pol_x_doubles(int rows, int width) { return (int64_t)uhc_pol_x_doubles(rows, width); }
EXPORT double pol_act(int code, double v) { return uhc_pol_act(code, v); }
EXPORT double pol_filter_denom(double n, double mean, double S) { return uhc_pol_filter_denom(n, mean, S); }
EXPORT double pol_filter(double x, double mean, double denom, int demean, int destd, double clip) { return uhc_pol_filter(x, mean, denom, demean, destd, clip); }

// what uhc_policy_pack_kernel does: slot by slot, the lane maps backwards
EXPORT void pol_pack(const double* W, const double* bias, int N, int K, double* wp, double* bp) {
    const int kpad = uhc_pol_pad4(K), npad = uhc_pol_pad16(N), ksteps = kpad >> 2;
    for (int64_t idx = 0; idx < (int64_t)npad * kpad; idx++) {
        const int lane = (int)(idx & 63), ks = (int)((idx >> 6) % ksteps), ct = (int)((idx >> 6) / ksteps);
        const int n = 16 * ct + uhc_pol_b_col(lane), k = uhc_pol_ab_k(lane, ks);
        wp[idx] = (n < N && k < K) ? W[(size_t)n * K + k] : 0.0;
    }
    for (int n = 0; n < npad; n++) bp[n] = n < N ? bias[n] : 0.0;
}

// One layer as the kernel runs it.  first: `in` is row-major [R][K] (the caller's observations), else the packed activation of the layer before.
// final: `out` is row-major [R][N], else the packed activation the next layer reads (every slot of the live row tiles is written).
EXPORT void pol_layer(int first, const double* in, int R, int K, const double* wp, const double* bp, int N, int act, int final, double* out) {
    const int ksteps = uhc_pol_pad4(K) >> 2, ntile = (R + 15) >> 4, nct = uhc_pol_pad16(N) >> 4, npad4 = uhc_pol_pad4(N);
    for (int rt = 0; rt < ntile; rt++)
        for (int ct = 0; ct < nct; ct++) {
            double acc[64][4] = {};
            for (int ks = 0; ks < ksteps; ks++) {
                double a[64], b[64];
                for (int lane = 0; lane < 64; lane++) {
                    b[lane] = wp[((size_t)ct * ksteps + ks) * 64 + lane];
                    if (first) {
                        const int r = 16 * rt + uhc_pol_a_row(lane), k = uhc_pol_ab_k(lane, ks);
                        a[lane] = (r < R && k < K) ? in[(size_t)r * K + k] : 0.0;
                    } else {
                        a[lane] = in[((size_t)rt * ksteps + ks) * 64 + lane];
                    }
                }
                // D[i][j] += sum_k A[i][k] B[k][j]: A[i][k] is lane 16 k + i's operand, B[k][j] lane 16 k + j's; D[i][j] is register i / 4 of lane 16 (i % 4) + j
                for (int lane = 0; lane < 64; lane++)
                    for (int reg = 0; reg < 4; reg++) {
                        const int i = uhc_pol_cd_row(lane, reg), j = uhc_pol_cd_col(lane);
                        for (int k = 0; k < 4; k++) acc[lane][reg] += a[16 * k + i] * b[16 * k + j];
                    }
            }
            for (int lane = 0; lane < 64; lane++)
                for (int reg = 0; reg < 4; reg++) {
                    const int r = 16 * rt + uhc_pol_cd_row(lane, reg), col = 16 * ct + uhc_pol_cd_col(lane);
                    const double v = uhc_pol_act(act, acc[lane][reg] + bp[col]);
                    if (final) {
                        if (r < R && col < N) out[(size_t)r * N + col] = v;
                    } else if (col < npad4) {
                        out[uhc_pol_x_index(r, col, npad4)] = col < N ? v : 0.0;
                    }
                }
        }
}
