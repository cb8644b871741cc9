// uhc_k_general_fwd.hip -- one translation unit of the fused step kernel (instantiations split across files so that they compile in parallel).
#include "uhc_physics_impl.h"
#include "uhc_launch.h"

UHC_ENV_LAUNCH(m1_gen, 1, 2, true)
UHC_ENV_LAUNCH(m2_gen, 2, 2, true)
