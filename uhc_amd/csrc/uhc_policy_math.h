// uhc_policy_math.h -- the arithmetic uhc_policy.hip shares with the host: where an element of a weight matrix, of an activation and of a layer's result lies in
// the operand order of v_mfma_f64_16x16x4_f64, the activation functions, and the observation filter's rule.  Plain C++ (the CPU tests compile it with the host
// compiler, tests/policy_pack_probe.cpp); under hipcc the functions are __host__ __device__.
//
// The instruction computes D[16][16] = A[16][4] B[4][16] + C with one double of A and one of B per lane, four of C / D:
//   A: lane l holds A[l & 15][l >> 4]        B: lane l holds B[l >> 4][l & 15]        C / D: lane l, register i holds C[(l >> 4) + 4 i][l & 15]
// (the f64 C / D map is not the f32 one).  A layer is Y = act(X W^T + b): A is a 16-row tile of X, B[k][n] = W[n][k] a 16-column tile of W^T.
//
//   packed weight      [column tile n / 16][k-step k / 4][lane = (k % 4) * 16 + n % 16], K padded to 4 and the output dimension to 16 with zeros:
//                      a wave's k-step is 64 consecutive doubles
//   packed activation  [row tile r / 16][k-step k / 4][lane = (k % 4) * 16 + r % 16], the width padded to 4 with zeros, the rows to 16
//   C / D -> next A    the result (row, col) of a layer is feature k = col of the next layer's input: uhc_pol_x_index(row, col, width padded to 4)
#pragma once
#include <math.h>
#include <stddef.h>

#ifdef __HIPCC__
#define UHC_POL_HD __host__ __device__ inline
#else
#define UHC_POL_HD inline
#endif

// activation codes of include/uhc_amd.h (UHC_ACT_*)
#define UHC_POL_ACT_NONE 0
#define UHC_POL_ACT_TANH 1
#define UHC_POL_ACT_RELU 2
#define UHC_POL_ACT_SIGMOID 3
#define UHC_POL_ACT_GELU 4
#define UHC_POL_N_ACT 5

UHC_POL_HD int uhc_pol_pad4(int k) { return (k + 3) & ~3; }
UHC_POL_HD int uhc_pol_pad16(int n) { return (n + 15) & ~15; }
UHC_POL_HD size_t uhc_pol_w_doubles(int out, int in) { return (size_t)uhc_pol_pad16(out) * uhc_pol_pad4(in); }
UHC_POL_HD size_t uhc_pol_x_doubles(int rows, int width) { return (size_t)uhc_pol_pad16(rows) * uhc_pol_pad4(width); }

// W[n][k] of an [out][in] matrix in the packed weight; kpad = uhc_pol_pad4(in)
UHC_POL_HD size_t uhc_pol_w_index(int n, int k, int kpad) { return ((size_t)(n >> 4) * (kpad >> 2) + (k >> 2)) * 64 + (size_t)((k & 3) * 16 + (n & 15)); }
// X[r][k] of a [rows][width] activation in the packed activation; kpad = uhc_pol_pad4(width)
UHC_POL_HD size_t uhc_pol_x_index(int r, int k, int kpad) { return ((size_t)(r >> 4) * (kpad >> 2) + (k >> 2)) * 64 + (size_t)((k & 3) * 16 + (r & 15)); }

// what lane `lane` feeds the instruction at k-step ks: its row within the tile and its k (A), its k and its column within the tile (B)
UHC_POL_HD int uhc_pol_a_row(int lane) { return lane & 15; }
UHC_POL_HD int uhc_pol_ab_k(int lane, int ks) { return 4 * ks + (lane >> 4); }
UHC_POL_HD int uhc_pol_b_col(int lane) { return lane & 15; }
// what register i of lane `lane` holds afterwards: row and column within the 16 x 16 tile
UHC_POL_HD int uhc_pol_cd_row(int lane, int i) { return (lane >> 4) + 4 * i; }
UHC_POL_HD int uhc_pol_cd_col(int lane) { return lane & 15; }

// The activations, as torch computes them in float64: nn.GELU() is the exact erf form, relu and the clip keep a NaN (comparisons, not fmin / fmax).
UHC_POL_HD double uhc_pol_act(int code, double v) {
    switch (code) {
        case UHC_POL_ACT_TANH: return tanh(v);
        case UHC_POL_ACT_RELU: return v < 0.0 ? 0.0 : v;
        case UHC_POL_ACT_SIGMOID: return 1.0 / (1.0 + exp(-v));
        case UHC_POL_ACT_GELU: return v * 0.5 * (1.0 + erf(v * 0.70710678118654752440));
        default: return v;
    }
}

// The observation filter, the arithmetic of uhc_filter_apply (ZFilter.__call__): y = clip((x - mean) / (std + 1e-8), +-clip), std = sqrt(S / (n - 1)), and
// |mean| while n <= 1 (RunningStat.var: np.square(mean)).  The denominator is formed once per column, the division (not a reciprocal) once per element.
UHC_POL_HD double uhc_pol_filter_denom(double n, double mean, double S) {
    const double var = n > 1.0 ? S / (n - 1.0) : mean * mean;
    return sqrt(var) + 1e-8;
}
UHC_POL_HD double uhc_pol_filter(double x, double mean, double denom, int demean, int destd, double clip) {
    double y = x;
    if (demean) y = y - mean;
    if (destd) y = y / denom;
    if (clip != 0.0) y = y < -clip ? -clip : (y > clip ? clip : y);
    return y;
}
