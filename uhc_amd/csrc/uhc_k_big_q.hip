// uhc_k_big_q.hip -- one translation unit of the fused step kernel: the large tier as a persistent consumer of an env queue (sticky tiers).
// (no tier 4 INSIDE this persistent consumer: an env beyond the large tier is flagged pend3 = 2 and appended to tier 4's own queue when that has consumers this step
//  -- uhc_k_huge_q.hip, four-wave workgroups --, else it stays flagged for the step's chained launch of uhc_k_big.hip, whose workgroup goes on with it as tier 4)
#include "uhc_physics_impl.h"
#include "uhc_launch.h"

UHC_QUEUE_LAUNCH(m0_big_q, 3, UHC_WAVE)
