// uhc_k_fast_dense.hip -- one translation unit of the fused step kernel (instantiations split across files so that they compile in parallel).
#include "uhc_physics_impl.h"
#include "uhc_launch.h"

UHC_ENV_LAUNCH(m0_fast_dense, 0, 1, true)
