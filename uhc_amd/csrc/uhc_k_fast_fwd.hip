// uhc_k_fast_fwd.hip -- one translation unit of the fused step kernel (instantiations split across files so that they compile in parallel).
#include "uhc_physics_impl.h"
#include "uhc_launch.h"

UHC_ENV_LAUNCH(m1_fast, 1, 1, false)
UHC_ENV_LAUNCH(m2_fast, 2, 1, false)
