// uhc_k_general.hip -- one translation unit of the fused step kernel (instantiations split across files so that they compile in parallel).
#include "uhc_physics_impl.h"
#include "uhc_launch.h"

UHC_ENV_LAUNCH(m0_gen, 0, 2, true)
