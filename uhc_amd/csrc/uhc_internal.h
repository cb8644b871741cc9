// uhc_internal.h -- the seams between the library's translation units: every uhc_launch_* symbol that uhc_launch.h's table does not generate, and every
// uhc_internal_* accessor but uhc_internal_set_error (uhc_api_check.h) and uhc_internal_batch_info (uhc_env_plan.h, with its struct).  Included by the unit that DEFINES a symbol and by every unit that CALLS it: they are
// extern "C", the linker compares names only, and a parameter added on one side alone would hand a kernel garbage pointers -- here it is a compile error
// ("conflicting types").  The types of the step (uhc_device.h) and of the env layer (uhc_device_env.h, uhc_expert_math.h) stand behind pointers, so the
// header reads neither and both sides include it; no step-kernel unit (uhc_k_*.hip) does.
#pragma once
#include <hip/hip_runtime.h>

struct DevState;     // uhc_device.h
struct EnvArgs;      // uhc_device_env.h
struct LiveState;    // uhc_expert_math.h
struct UhcBatch;     // uhc_host.h

extern "C" {
// ------------------------------------------------------------------ uhc_batch_kernels.hip, called by uhc_capi.cpp
hipError_t uhc_launch_tier_lists(const int* tier, const int* d_active, int n_env, int* tier_now, int* lists, int* counts, int* cursors, int* fin, const int* cost,
                                 const int* fresh, int* order, int launch4, int* pend3, hipStream_t stream);
hipError_t uhc_launch_gate(const int* started, int want, int* waited, long long* trace, hipStream_t stream);
hipError_t uhc_launch_set_state(const DevState* s, int nq, int nv, int nu, const int* env_ids, int n, const double* qpos, const double* qvel, int* mask,
                                hipStream_t stream);
hipError_t uhc_launch_set_state_masked(const DevState* s, int nq, int nv, int nu, int n_env, const int* select, const double* qpos, const double* qvel,
                                       int* mask, hipStream_t stream);
// ------------------------------------------------------------------ uhc_env.hip, called by uhc_env_capi.cpp
hipError_t uhc_launch_env_pre(const EnvArgs* E, const int* d_active, hipStream_t s);
hipError_t uhc_launch_env_post(int mode, const EnvArgs* E, const double* d_action, const int* d_active, hipStream_t s);
hipError_t uhc_launch_env_reset_stage(const EnvArgs* E, const int* env_ids, int n, const double* noise, double* out_qpos, double* out_qvel, hipStream_t s);
hipError_t uhc_launch_env_assign(const EnvArgs* E, const int* env_ids, int n, const int* clip_ids, const int* fr_start, const int* fr_len, hipStream_t s);
hipError_t uhc_launch_env_set_next(const EnvArgs* E, const int* env_ids, int n, const int* clip_ids, const int* fr_start, const int* fr_len, const double* noise,
                                   hipStream_t s);
hipError_t uhc_launch_env_auto_stage(const EnvArgs* E, double* out_qpos, double* out_qvel, int* select, hipStream_t s);
// ------------------------------------------------------------------ uhc_live.hip, called by uhc_env_capi.cpp
hipError_t uhc_launch_live_push(const EnvArgs* E, const LiveState* L, const int* env_ids, int n, const double* qpos, const double* root_record,
                                const int* restart, const int* model, hipStream_t s);
// ------------------------------------------------------------------ uhc_capi.cpp: what the env layer (uhc_env_capi.cpp) reads of a batch
// (the batch's dims: uhc_internal_batch_info, declared beside the struct it returns -- uhc_env_plan.h, which a host build without the HIP headers reads too)
hipStream_t uhc_internal_stream(UhcBatch* b);  // read per call: uhc_batch_set_stream may change it
int* uhc_internal_reset_mask(UhcBatch* b);     // [n_env] the envs of the last uhc_batch_set_state
int* uhc_internal_env_model(UhcBatch* b, int* n_models);
int uhc_internal_set_state_masked(UhcBatch* b, const int* d_select, const double* d_qpos, const double* d_qvel);
}
