// uhc_seq.h -- the sequence rules of the post-processing units (uhc_expert.hip, uhc_eval.hip, uhc_smpl.hip, uhc_surface.hip, uhc_smpl_mesh.hip, uhc_live.hip),
// one definition each.  What this header owns is one promise: NO INDEX, WHATEVER IT HOLDS, LEAVES THE ARRAYS.  Row counts, first rows, model indices and clip
// tables arrive from device memory the caller filled; each is brought into its range (or its sequence skipped) here, before it forms an address.
//
// Plain integer and float64 functions on scalars and pointers: nothing of the HIP runtime, nothing of the step headers.  Those without a lane operation are
// __host__ __device__, so that tests/seq_probe.cpp compiles them with the host compiler; the xor butterflies at the end are device code and want
// <hip/hip_runtime.h> included in front of this header.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define UHC_SEQ_HD __host__ __device__ __forceinline__
#else
#define UHC_SEQ_HD inline
#endif

// the quiet NaN every unit writes for "no value": np.mean of an empty array, a row with a non-finite input
UHC_SEQ_HD double uhc_nan() { return __builtin_bit_cast(double, 0x7ff8000000000000LL); }

// a sequence's row count, clamped to 0 .. row_cap: whatever the counter holds, the rows read lie inside the arrays
UHC_SEQ_HD int uhc_seq_rows(int r, int row_cap) { return r < 0 ? 0 : (r > row_cap ? row_cap : r); }

// a sequence's first global row g, or -1 when its T rows would leave 0 .. n_rows_total (the sequence is then skipped)
UHC_SEQ_HD long long uhc_seq_start(long long g, int T, long long n_rows_total) { return g >= 0 && g <= n_rows_total - T ? g : -1; }

// a model index: one outside 0 .. n_models - 1 reads as 0; a table that is NULL names model 0 for every entry
UHC_SEQ_HD int uhc_seq_model(int m, int n_models) { return m >= 0 && m < n_models ? m : 0; }
UHC_SEQ_HD int uhc_seq_model(const int* model, long long s, int n_models) { return uhc_seq_model(model ? model[s] : 0, n_models); }

// the clip of frame f: the last clip whose start is <= f (clip 0 for a frame below every start).  The result stays inside 0 .. n_clips - 1 whatever the table
// holds: one that is not ascending can name the wrong clip, never an address outside the arrays.  n_clips >= 1.
UHC_SEQ_HD int uhc_clip_of(const int* clip_start, int n_clips, long long f) {
    int lo = 0, hi = n_clips - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long long)clip_start[mid] <= f) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// byte i (0 .. 23) of a table that travels as three kernel-argument words: no array is indexed at run time
UHC_SEQ_HD int uhc_packed_byte(const unsigned long long (&w)[3], int i) {
    const unsigned long long v = i < 8 ? w[0] : (i < 16 ? w[1] : w[2]);
    return (int)((v >> (8 * (i & 7))) & 0xff);
}

// the mean of column k over the n rows g0 .. g0 + n - 1 of rows [..][stride], summed in row order; NaN over no row (np.mean of an empty array; n <= 0)
UHC_SEQ_HD double uhc_seq_mean(const double* rows, int stride, int k, long long g0, int n) {
    n = n < 0 ? 0 : n;
    double s = 0.0;
    for (int r = 0; r < n; r++) s += rows[(size_t)(g0 + r) * stride + k];
    return n > 0 ? s / n : uhc_nan();
}

#if defined(__HIPCC__)
// Xor butterflies over the 2 FIRST_MASK lanes of the caller's group (FIRST_MASK, .., 2, 1): every lane ends with the same bits, in an order fixed by the lane
// numbers alone.  32: the wave; 16: a half; 8: a group of 16.
template <int FIRST_MASK, class T>  // T: double or int
__device__ __forceinline__ T uhc_xor_sum(T v) {
#pragma unroll
    for (int m = FIRST_MASK; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
template <int FIRST_MASK>
__device__ __forceinline__ double uhc_xor_min(double v) {
#pragma unroll
    for (int m = FIRST_MASK; m >= 1; m >>= 1) {
        const double o = __shfl_xor(v, m);
        v = o < v ? o : v;
    }
    return v;
}
#endif
