// uhc_k_big.hip -- one translation unit of the fused step kernel (instantiations split across files so that they compile in parallel).
// the large tier's workgroups go on as tier 4 (Newton on the primal, uhc_primal.h) when an env does not fit or its working sets give up
#define UHC_WITH_TIER4
#include "uhc_physics_impl.h"
#include "uhc_launch.h"

UHC_ENV_LAUNCH(m0_big, 0, 3, true)
