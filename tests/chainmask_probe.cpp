// chainmask_probe.cpp -- tests/plan_probe.cpp plus one accessor: the planner's chain masks (BatchPlan::chainmask, uploaded as DevTopo::dof_chainmask) of the plan probed
// last, for tests/test_delassus_tiles_cpu.py, which compares them with the same plan's dof_anc.  Built with the host compiler, together with uhc_plan.cpp.
#include "plan_probe.cpp"

// -> number of 64-bit words ([nv][2]); out (may be NULL) receives up to cap of them
PROBE long long uhc_plan_probe_chainmask(unsigned long long* out, long long cap) {
    const std::vector<unsigned long long>& m = g_plan.chainmask;
    for (long long k = 0; out && k < (long long)m.size() && k < cap; k++) out[k] = m[k];
    return (long long)m.size();
}
