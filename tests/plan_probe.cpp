// plan_probe.cpp -- thin C interface over uhc_plan.cpp for tests/test_batch_plan_cpu.py: built with the host compiler, no HIP runtime.
#include <algorithm>
#include <cstdlib>

#include "uhc_plan.h"

struct PlanView {  // what the probe reports of a plan
    const KernelArgs* A;
    long long lds_bytes, lds_bytes_fast, lds_bytes_big;
    int use_fast, n_trailing_free, q2_div, q2_wait_min, q2_max, q3_max, q4_max;
};
struct Table { const char* name; const void* p; long long bytes; };
// the plan as (name, value) words: every pointer-free field of KernelArgs that batch creation decides, and the batch's launch sizes and caps
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
typedef std::vector<std::pair<std::string, int64_t>> Words;
static int64_t dbits(double x) { int64_t v; memcpy(&v, &x, 8); return v; }
static void put_ints(Words& w, const char* prefix, const char* names, const int* p) {  // names: "a, b, c" as in the struct's declaration
    std::string s(names);
    size_t at = 0;
    for (int k = 0; at < s.size(); k++) {
        size_t e = s.find(',', at);
        if (e == std::string::npos) e = s.size();
        std::string n = s.substr(at, e - at);
        while (!n.empty() && n[0] == ' ') n.erase(0, 1);
        w.push_back({std::string(prefix) + n, p[k]});
        at = e + 1;
    }
}
#define LDS_NAMES "qpos, qvel, qacc, ctrl, applied, xpos, xquat, xmat, xipos, ximat, rootcom, cinert, crb, cvel, cacc, cfrc, xanchor, xaxis, cdof, cdofdot, M, LD, dinv, sdinv, bias, smooth, vec, z, zero, mij, con, Y, rowR, rowAref, rowB, rowF, rowDa, rowMisc, ncon_nefc, rowW, rowY, dense, dcol, dsc, H, total"
#define OFF_NAMES "body_pos, body_quat, body_ipos, body_iquat, body_mass, body_inertia, body_invweight0, jnt_pos, jnt_axis, jnt_range, jnt_stiffness, jnt_margin, qpos0, qpos_spring, dof_armature, dof_damping, dof_frictionloss, dof_invweight0, geom_pos, geom_quat, geom_friction, geom_margin, geom_gap, geom_solref, geom_solimp, geom_rbound, geom_center, geom_box, geom_radius, mesh_vert, actuator_gear, meaninertia, mesh_adj, stride"
#define CAP_NAMES "maxefc, maxcon, ndense, ycap, vstage, ld_delta"
static_assert(sizeof(DevLds) == 46 * sizeof(int) && sizeof(DevNumOff) == 34 * sizeof(int) && sizeof(TierCap) == 6 * sizeof(int), "the name lists above follow uhc_device.h");
static Words plan_words(const PlanView& v) {
    const KernelArgs& A = *v.A;
    const DevTopo& T = A.t;
    Words w;
    put_ints(w, "t.", "nq, nv, nu, nbody, njnt, ngeom, nM, maxdepth, nmeshvert, npair, iterations, plane_mesh_maxcon, solver", &T.nq);
    w.push_back({"t.timestep", dbits(T.timestep)}); w.push_back({"t.tolerance", dbits(T.tolerance)});
    for (int k = 0; k < 3; k++) w.push_back({"t.gravity" + std::to_string(k), dbits(T.gravity[k])});
    w.push_back({"t.ncpair", T.ncpair}); w.push_back({"t.body_maxdepth", T.body_maxdepth}); w.push_back({"t.fac_nslot", T.fac_nslot}); w.push_back({"t.has_damping", T.has_damping});
    put_ints(w, "o.", OFF_NAMES, &A.o.body_pos);
    put_ints(w, "lf.", LDS_NAMES, &A.lf.qpos); put_ints(w, "l.", LDS_NAMES, &A.l.qpos); put_ints(w, "lh.", LDS_NAMES, &A.lh.qpos); put_ints(w, "lx.", LDS_NAMES, &A.lx.qpos);
    put_ints(w, "cf.", CAP_NAMES, &A.cf.maxefc); put_ints(w, "cg.", CAP_NAMES, &A.cg.maxefc); put_ints(w, "ch.", CAP_NAMES, &A.ch.maxefc); put_ints(w, "cx.", CAP_NAMES, &A.cx.maxefc);
    w.push_back({"gy_stride", A.gy_stride}); w.push_back({"gd_stride", A.gd_stride}); w.push_back({"last_tier", A.last_tier});
    for (int k = 0; k < 8; k++) w.push_back({"marks" + std::to_string(k), A.marks[k]});
    w.push_back({"t4_rows", A.t4_rows}); w.push_back({"ball_limits", A.ball_limits}); w.push_back({"dbg", A.dbg}); w.push_back({"nvp", A.nvp}); w.push_back({"adjdeg", A.adjdeg});
    put_ints(w, "c.", "n_substeps, action_type, meta_pd, rfc_mode, action_dim, n_vf_body, body_vf_dim", &A.c.n_substeps);
    w.push_back({"c.rfc_scale", dbits(A.c.rfc_scale)}); w.push_back({"c.rfc_lim", dbits(A.c.rfc_lim)});
    for (int k = 0; k < 4; k++) w.push_back({"c.base_rot_inv" + std::to_string(k), dbits(A.c.base_rot_inv[k])});
    w.push_back({"n_env", A.n_env});
    w.push_back({"lds_bytes", v.lds_bytes}); w.push_back({"lds_bytes_fast", v.lds_bytes_fast}); w.push_back({"lds_bytes_big", v.lds_bytes_big});
    w.push_back({"use_fast", v.use_fast}); w.push_back({"n_trailing_free", v.n_trailing_free});
    w.push_back({"q2_div", v.q2_div}); w.push_back({"q2_wait_min", v.q2_wait_min}); w.push_back({"q2_max", v.q2_max}); w.push_back({"q3_max", v.q3_max}); w.push_back({"q4_max", v.q4_max});
    return w;
}

static BatchPlan g_plan;
template <class T>
static Table table_of(const char* name, const std::vector<T>& v) { return Table{name, v.data(), (long long)(v.size() * sizeof(T))}; }
static int run_plan(const UhcModelDesc* md, int n_env, const UhcCtrlDesc* ctrl, std::string* err, PlanView* v, std::vector<Table>* tabs) {
    UhcModel m;
    m.d = *md;  // (the planner reads the description only; the caller's arrays outlive the call)
    const UhcModel* ms[1] = {&m};
    const BatchKnobs k = read_knobs();
    if (plan_batch(ms, 1, nullptr, n_env, ctrl, k, &g_plan, err)) return 1;
    const BatchPlan& P = g_plan;
    *v = PlanView{&P.A, (long long)P.lds_bytes, (long long)P.lds_bytes_fast, (long long)P.lds_bytes_big, P.use_fast, P.n_trailing_free, k.q2_div, k.q2_wait_min, k.q2_max, k.q3_max, k.q4_max};
    *tabs = {table_of("body_depth", P.body_depth), table_of("body_rootid", P.body_rootid), table_of("body_nsub", P.body_nsub), table_of("body_lastdof", P.body_lastdof),
             table_of("dof_depth", P.dof_depth), table_of("dof_ndesc", P.dof_ndesc), table_of("dof_anc", P.dof_anc), table_of("m_row", P.m_row), table_of("m_col", P.m_col),
             table_of("m_ij", P.m_ij), table_of("ncommon", P.ncommon), table_of("dof_rootid", P.dof_rootid), table_of("pg1", P.pg1), table_of("pg2", P.pg2),
             table_of("cg1", P.cg1), table_of("cg2", P.cg2), table_of("model_blob", P.model_blob), table_of("fac_prog", P.fac_prog), table_of("sol_back", P.sol_back),
             table_of("sol_fwd", P.sol_fwd), table_of("chain", P.chain), table_of("dof_act", P.dof_act), table_of("guard_tab", P.guard_tab), table_of("vf_body", P.vf_body)};
    return 0;
}
// in: est2, est3, est4, est2_then, handed2, n_env, n_cu, lds_bytes_fast, large_first, last_tier, queues_off, q2_div, q2_wait_min, q2_max, q3_max, q4_max, UHC_DEBUG word
static void put_sticky(const StickySizes& s, int* out) {
    const int o[10] = {s.queues, s.waiting, s.q3, s.q4, s.launch4, s.grid2, s.grid3, s.grid4, s.n_wait, s.sticky_mask};
    memcpy(out, o, sizeof o);
}
// (the list kernel's decision and the sizes from one queues_off: a step in which the back-off does not flip)
static StickyInputs sticky_inputs(const int* in) {
    return StickyInputs{in[0], in[1], in[2], in[3], in[4], in[5], in[6], (size_t)in[7], in[8] != 0, in[9], in[10] != 0, in[11], in[12], in[13], in[14], in[15], (in[16] & 2048) != 0};
}
static void run_sticky(const int* in, int* out) { put_sticky(plan_sticky_step(sticky_inputs(in)), out); }
// in: the 17 words above, n_substeps, fast_chunk, the queues_off the step BEGAN with (what the list kernel's decision saw; in[10] is the one after the back-off
// update).  out: the 10 words of run_sticky; the fast tier's chunk, n_chunks, grid, prod_total; the number of launches;
// per launch WIRING_WORDS words in the order of StepLaunch's declaration
#define WIRING_WORDS 20
static void run_wiring(const int* in, int* out) {
    StickyInputs si = sticky_inputs(in);
    si.n_substeps = in[17]; si.fast_chunk = in[18];
    const StickySizes s = plan_sticky_step(si, sticky_launch4(si.last_tier, si.est4, si.est2_then, in[19] != 0));
    const StepWiring w = sticky_wiring(s, si.large_first);
    put_sticky(s, out);
    out[10] = s.fast.chunk; out[11] = s.fast.n_chunks; out[12] = s.fast.grid; out[13] = s.fast.prod_total; out[14] = w.n;
    for (int k = 0; k < 4; k++) {
        const StepLaunch& l = w.launch[k];
        const int o[WIRING_WORDS] = {l.tier, l.stream, l.list, l.count, l.cursor, l.grid, l.n_wait, l.spares, l.started, l.prod_fin, l.prod_total, l.fin, l.next_list, l.next_count,
                                     l.gate_started, l.gate_want, l.gate_waited, l.tier_want, l.chunk, l.use_order};
        memcpy(out + 15 + WIRING_WORDS * k, o, sizeof o);
    }
}
// C interface of the probe (tests/test_batch_plan_cpu.py): one plan at a time, kept until the next call
static Words g_words;
static std::vector<Table> g_tabs;
static std::string g_names, g_tnames, g_perr;
static uint64_t fnv64(const void* p, long long n) {
    uint64_t h = 1469598103934665603ull;
    for (long long i = 0; i < n; i++) { h ^= ((const unsigned char*)p)[i]; h *= 1099511628211ull; }
    return h;
}
// knobs: "UHC_TIERS=2;UHC_GUARD_LDS=1" -- set in the environment for this one call (batch creation reads its knobs there)
extern "C" __attribute__((visibility("default"))) int uhc_plan_probe(const UhcModelDesc* md, int n_env, const UhcCtrlDesc* ctrl, const char* knobs) {
    std::vector<std::string> set;
    std::string k(knobs ? knobs : "");
    for (size_t at = 0; at < k.size();) {
        size_t e = k.find(';', at);
        if (e == std::string::npos) e = k.size();
        const std::string kv = k.substr(at, e - at);
        const size_t eq = kv.find('=');
        if (eq != std::string::npos) { setenv(kv.substr(0, eq).c_str(), kv.substr(eq + 1).c_str(), 1); set.push_back(kv.substr(0, eq)); }
        at = e + 1;
    }
    g_words.clear(); g_tabs.clear(); g_perr.clear();
    PlanView v;
    const int rc = run_plan(md, n_env, ctrl, &g_perr, &v, &g_tabs);
    for (auto& n : set) unsetenv(n.c_str());
    if (rc) return rc;
    g_words = plan_words(v);
    g_names.clear(); g_tnames.clear();
    for (auto& w : g_words) g_names += w.first + ",";
    for (auto& t : g_tabs) g_tnames += std::string(t.name) + ",";
    return 0;
}
extern "C" __attribute__((visibility("default"))) const char* uhc_plan_probe_error(void) { return g_perr.c_str(); }
extern "C" __attribute__((visibility("default"))) const char* uhc_plan_probe_word_names(void) { return g_names.c_str(); }
extern "C" __attribute__((visibility("default"))) const char* uhc_plan_probe_table_names(void) { return g_tnames.c_str(); }
extern "C" __attribute__((visibility("default"))) int uhc_plan_probe_words(int64_t* out, int cap) {
    for (int k = 0; k < (int)g_words.size() && k < cap; k++) out[k] = g_words[k].second;
    return (int)g_words.size();
}
// -> bytes of the table (-1: no such table); hash = 64-bit FNV-1a of them; out (may be NULL) receives up to cap bytes
extern "C" __attribute__((visibility("default"))) long long uhc_plan_probe_table(const char* name, uint64_t* hash, void* out, long long cap) {
    for (auto& t : g_tabs)
        if (!strcmp(t.name, name)) {
            if (hash) *hash = fnv64(t.p, t.bytes);
            if (out) memcpy(out, t.p, (size_t)std::min(cap, t.bytes));
            return t.bytes;
        }
    return -1;
}
extern "C" __attribute__((visibility("default"))) void uhc_plan_probe_sticky(const int* in17, int* out10) { run_sticky(in17, out10); }
extern "C" __attribute__((visibility("default"))) void uhc_plan_probe_wiring(const int* in20, int* out95) { run_wiring(in20, out95); }

// ---- the step's words and the tier policy (uhc_step_words.h) for tests/test_step_words_cpu.py, on the marks and capacities of the plan probed last
// last_tier, t4_rows < 0: the plan's own
static KernelArgs args_with(int last_tier, int t4_rows) {
    KernelArgs A = g_plan.A;
    if (last_tier >= 0) A.last_tier = last_tier;
    if (t4_rows >= 0) A.t4_rows = t4_rows;
    return A;
}
#define PROBE extern "C" __attribute__((visibility("default")))
PROBE int uhc_sw_next_tier(int tier, const int* pk, int last_tier, int t4_rows, int sticky4) { return next_tier(tier, pk[0], pk[1], pk[2], pk[3], pk[4], args_with(last_tier, t4_rows), sticky4 != 0); }
PROBE int uhc_sw_launch_cost(const int* pk, double vmax_end) { return launch_cost(pk[0], pk[1], pk[2], pk[3], vmax_end, g_plan.A); }
PROBE int uhc_sw_redo_word(int tier, int status, int swept_mask) { return redo_word(tier, status, swept_mask); }
PROBE int uhc_sw_redo_written(int tier, int status) { return redo_written(tier, status) ? 1 : 0; }
PROBE int uhc_sw_swept_mask(int mask, int status, int it) { return redo_swept_mask(mask, status, it); }
// (as k_forward puts them together; exact: solver 1, the sweeps are the fallback of the working sets)
PROBE int uhc_sw_ws_gave_up_status(int exact, int code) { return UHC_ST_SWEPT | ((exact && code != UHC_WS_LOST) ? UHC_WS_REASON(code) : 0); }
PROBE int uhc_sw_handon_why_word(int tier, int old_word, int status, int substep) { return handon_why_word(tier, old_word, status, substep); }
PROBE int uhc_sw_order_bucket(int tier, int masked, int active, int fresh, int cost) { return order_bucket(&tier, masked != 0, &active, &fresh, &cost, 0); }
// (as uhc_tier_lists_kernel puts the two rules together)
PROBE int uhc_sw_start_tier(int tier, int fresh, int launch4) {
    const int t = start_tier(tier, &fresh, 0);
    return t == 4 ? start_tier4(launch4 != 0) : t;
}
// pk[5], *status: merged in place with the record rec[UHC_CHUNK_REC], word by word as uhc_step_env does
PROBE void uhc_sw_chunk_rec_merge(int* pk, int* status, const int* rec) {
    const int words[5] = {UHC_REC_PK_NEFC, UHC_REC_PK_NCON, UHC_REC_PK_NTWO, UHC_REC_PK_Y, UHC_REC_PK_ACT};
    for (int k = 0; k < 5; k++) pk[k] = chunk_rec_merged(words[k], pk[k], rec[words[k]]);
    *status = chunk_rec_merged(UHC_REC_STATUS, *status, rec[UHC_REC_STATUS]);
}
// the names the test needs by value: the status bits in UhcStatus's order, UHC_WHY_SHIFT, k_as_general's give-up codes, the record's words, UHC_ORDER_BUCKETS
PROBE void uhc_sw_names(int* out) {
    const int o[26] = {UHC_ST_HANDON, UHC_ST_DROPPED, UHC_ST_SWEPT, UHC_ST_WHY_FRICTION, UHC_ST_WINDOWED, UHC_ST_WHY_NOCONV, UHC_ST_WHY_PIVOT, UHC_ST_PRIMAL, UHC_ST_PRIMAL_CAP,
                       UHC_WHY_SHIFT, UHC_WS_FRICTION, UHC_WS_LOST, UHC_WS_NOCONV, UHC_WS_PIVOT, UHC_WS_TIER4,
                       UHC_REC_PK_NEFC, UHC_REC_PK_NCON, UHC_REC_PK_NTWO, UHC_REC_PK_Y, UHC_REC_PK_ACT, UHC_REC_NCON, UHC_REC_NEFC, UHC_REC_ITERS, UHC_REC_STATUS, UHC_CHUNK_REC,
                       UHC_ORDER_BUCKETS};
    memcpy(out, o, sizeof o);
}
