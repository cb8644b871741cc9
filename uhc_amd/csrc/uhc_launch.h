// uhc_launch.h -- the instantiations of the fused step kernel: each lives in a translation unit of its own (uhc_k_*.hip, so that they compile in parallel)
// behind a launcher and a setter of its dynamic-LDS limit; the host picks one from the table below.  The uhc_launch_* symbols stay inside the library.
#pragma once
#include <hip/hip_runtime.h>

#include "uhc_device.h"

typedef hipError_t (*UhcStepLaunch)(const KernelArgs* A, const double* d_action, const double* d_tbase, const int* d_active, size_t lds_bytes, hipStream_t stream);
typedef hipError_t (*UhcSetLds)(size_t lds_bytes);

// every instantiation, once: X(name, mode, tier, dense, queue)
// mode 0: control step, 1: forward only, 2: kinematics only; tier 1: the fast kernel, 2: general, 3: large, 4: tier 4; dense: the instantiation carries body-body
// rows (fast tier: the model has body-body contacts or limited ball joints; the larger tiers always do); queue: a persistent consumer of an env queue (sticky tiers)
#define UHC_STEP_INSTANCES(X)                                                                                                                     \
    X(m0_fast, 0, 1, false, false) X(m0_fast_dense, 0, 1, true, false) X(m1_fast, 1, 1, false, false) X(m1_fast_dense, 1, 1, true, false)         \
    X(m2_fast, 2, 1, false, false) X(m0_gen, 0, 2, true, false) X(m1_gen, 1, 2, true, false) X(m2_gen, 2, 2, true, false)                         \
    X(m0_big, 0, 3, true, false) X(m1_big, 1, 3, true, false) X(m0_gen_q, 0, 2, true, true) X(m0_big_q, 0, 3, true, true) X(m0_huge_q, 0, 4, true, true)

#define UHC_DECL_LAUNCH(name, mode, tier, dense, queue)                                                                                         \
    extern "C" hipError_t uhc_launch_##name(const KernelArgs* A, const double* d_action, const double* d_tbase, const int* d_active, size_t lds_bytes, \
                                            hipStream_t stream);                                                                                 \
    extern "C" hipError_t uhc_launch_##name##_lds(size_t lds_bytes);
UHC_STEP_INSTANCES(UHC_DECL_LAUNCH)

// in uhc_k_*.hip: the launcher of KERNEL<MODE, TIER, DENSE> and the setter of its LDS limit.  GRID: workgroups; the trailing arguments follow
// (*A, d_action, d_tbase) in the kernel's parameter list
#define UHC_DEFINE_LAUNCH(name, KERNEL, MODE, TIER, DENSE, THREADS, GRID, ...)                                                                        \
    extern "C" hipError_t uhc_launch_##name(const KernelArgs* A, const double* d_action, const double* d_tbase, const int* d_active, size_t lds_bytes, \
                                            hipStream_t stream) {                                                                                     \
        (void)d_active;                                                                                                                               \
        hipLaunchKernelGGL((KERNEL<MODE, TIER, DENSE>), dim3(GRID), dim3(THREADS), lds_bytes, stream, *A, d_action, d_tbase, ##__VA_ARGS__);          \
        return hipGetLastError();                                                                                                                     \
    }                                                                                                                                                 \
    extern "C" hipError_t uhc_launch_##name##_lds(size_t lds_bytes) {                                                                                 \
        return hipFuncSetAttribute((const void*)KERNEL<MODE, TIER, DENSE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);               \
    }
// one workgroup per env (or per entry of a launch order): the active mask goes to the kernel
#define UHC_ENV_LAUNCH(name, MODE, TIER, DENSE) UHC_DEFINE_LAUNCH(name, uhc_step_kernel, MODE, TIER, DENSE, UHC_WAVE, A->grid ? A->grid : A->n_env, d_active)
// queue consumers (mode 0): A->grid persistent workgroups; the queue says which envs, d_active is not read
#define UHC_QUEUE_LAUNCH(name, TIER, THREADS) UHC_DEFINE_LAUNCH(name, uhc_step_queue_kernel, 0, TIER, true, THREADS, A->grid)

// host side: one row per instantiation; lds = which of the batch's three LDS sizes its limit is (0 general, 1 fast, 2 large / tier 4)
struct UhcStepInstance { int mode, tier; bool dense, queue; UhcStepLaunch launch; UhcSetLds set_lds; int lds; };
#define UHC_INSTANCE_ROW(name, mode, tier, dense, queue) {mode, tier, dense, queue, uhc_launch_##name, uhc_launch_##name##_lds, tier == 1 ? 1 : tier == 2 ? 0 : 2},
#define UHC_STEP_TABLE {UHC_STEP_INSTANCES(UHC_INSTANCE_ROW)}
