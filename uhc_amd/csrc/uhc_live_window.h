// uhc_live_window.h -- the window rule of a sliding live stream (include/uhc_amd.h, "live targets": uhc_env_live_slide), shared by the device kernel
// (uhc_live.hip: uhc_live_slide_kernel) and a host build (tests/live_window_probe.cpp).  Integer arithmetic on four values: nothing of the HIP runtime.
//
// An env's stream is a slice of `cap` records; `len` of them are filled.  The env kernels (uhc_env.hip) find frame t of the env at local index
// min(start_ind + t, len - 1) and read t = cur_t (observation v0), cur_t + 1 (PD target, reward, observation) and the look-aheads behind it: the lowest
// local index that can still be read is start_ind + cur_t.  A slide discards the S oldest records, moves the others to the front of the slice and subtracts
// S from start_ind and len, so every later read resolves to the same global frame: min(start_ind - S + t, len - S - 1) + S == min(start_ind + t, len - 1).
//
//   uhc_lw_discard  S, the number of records to discard ahead of an append:
//                     0 unless len == cap (a slide happens only when the slice is full);
//                     otherwise min(max(start_ind + cur_t, 0), len - 1): everything behind the consumer goes, the newest record always stays (a stream
//                     that has run dry keeps holding it).
//                   S == 0 on a full slice means the consumer has not moved: the append is dropped and counted, as without sliding.
//
// Invariant: start_ind + cur_t >= 0 always holds.  uhc_env_reset sets both to 0, a step adds 1 to cur_t, and a slide subtracts S <= start_ind + cur_t from
// start_ind.  So no index derived from the sum ever leaves the slice [0, len - 1] -- also between a restart row (which sets len = 1 and leaves start_ind and
// cur_t as they are) and the uhc_env_reset that follows it.  The max(., 0) above costs nothing and keeps S in range on memory that does not hold the invariant.
#pragma once

#if defined(__HIPCC__)
#define UHC_LW_HD __host__ __device__ __forceinline__
#else
#define UHC_LW_HD inline
#endif

UHC_LW_HD int uhc_lw_discard(int len, int cap, int start_ind, int cur_t) {
    if (len != cap || len < 1) return 0;
    // (64-bit: the sum of two ints read from memory cannot wrap)
    long long behind = (long long)start_ind + (long long)cur_t;
    if (behind < 0) behind = 0;
    return behind < (long long)(len - 1) ? (int)behind : len - 1;
}
