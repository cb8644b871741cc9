// uhc_k_general_q.hip -- one translation unit of the fused step kernel: the general tier as a persistent consumer of an env queue (sticky tiers).
// Its workgroups have TWO waves (UHC_NW2): wave 0 runs the step like every other tier's workgroup, wave 1 serves every second group of support requests of the MPR
// rounds (uhc_mpr.h: mpr_wave_mw) -- two 79 KiB consumers share a CU, so two of its four SIMDs were idle, and the slowest general-tier env is what the headline's step waits for.
#define UHC_NW2
#include "uhc_physics_impl.h"
#include "uhc_launch.h"

UHC_QUEUE_LAUNCH(m0_gen_q, 2, UHC_QUEUE_THREADS)
