// uhc_api_check.h -- the host side every C entry of the post-processing units and of the env layer shares: how a call is refused (by name, before the first HIP
// call), how a failed HIP call is reported, and the few steps around a launch that each entry used to spell out for itself.  uhc_capi.cpp owns the error
// string (uhc_last_error) and reports its own failed HIP calls through the same macro.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

// uhc_capi.cpp (which includes this header too): keeps the text for uhc_last_error, returns 1.  Declared here, not in uhc_internal.h: uhc_rollout.hip reads this header alone
extern "C" int uhc_internal_set_error(const char* msg);

#define HIP_OK(expr)                                                                                                          \
    do {                                                                                                                      \
        hipError_t e__ = (expr);                                                                                              \
        if (e__ != hipSuccess) return uhc_internal_set_error((std::string(#expr) + ": " + hipGetErrorString(e__)).c_str()); \
    } while (0)

// "<fn>: <what>" and out, when cond holds; fn and what may each be a literal or a run-time string
#define REFUSE(fn, cond, what) \
    if (cond) return uhc_internal_set_error((std::string(fn) + ": " + (what)).c_str())

// a grid's x extent is an int
static inline bool uhc_launch_fits(long long blocks) { return blocks <= 0x7fffffffLL; }

// The tail of an entry that counts bad rows in d_bad: a caller that passes h_bad wants the count now.  The one place that waits for the stream.
static inline int uhc_return_bad(int32_t* h_bad, const int32_t* d_bad, hipStream_t s) {
    if (h_bad) {
        HIP_OK(hipMemcpyAsync(h_bad, d_bad, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
    }
    return 0;
}

// a host table of n entries into device memory of its own (*dst is the caller's to free, also after a failure)
template <class T>
static hipError_t uhc_upload(T** dst, const T* src, size_t n) {
    hipError_t e = hipMalloc((void**)dst, sizeof(T) * n);
    if (e == hipSuccess) e = hipMemcpy(*dst, src, sizeof(T) * n, hipMemcpyHostToDevice);
    return e;
}

static inline bool uhc_all_finite(const double* p, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(p[i])) return false;
    return true;
}
