// uhc_capi.cpp -- host side of libuhc_amd.so: the C-ABI declared in include/uhc_amd.h.
// Owns model copies, device buffers and kernel launches; what a batch looks like is decided in uhc_plan.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "uhc_host.h"
#include "uhc_launch.h"
#include "uhc_plan.h"

static const UhcStepInstance g_steps[] = UHC_STEP_TABLE;
// the instantiation for (mode, tier) of this launch: queue consumers (mode 0, tiers 2 / 3 / 4) when the launch has a list; the fast tier's DENSE
// instantiation when the model has body-body contacts or limited ball joints (the instantiation that carries their rows)
static hipError_t uhc_launch_step(int mode, int tier, const KernelArgs* A, const double* d_action, const double* d_tbase, const int* d_active,
                                  size_t lds_bytes, hipStream_t stream) {
    const bool queue = A->list != nullptr;
    if (queue) { mode = 0; tier = tier == 4 ? 4 : tier == 3 ? 3 : 2; }
    else if (tier == 3) mode = mode == 0 ? 0 : 1;  // (the large tier has no kinematics-only instantiation: forward)
    else if (tier != 1) { tier = 2; mode = mode == 0 ? 0 : mode == 1 ? 1 : 2; }
    else mode = mode == 2 ? 2 : mode == 0 ? 0 : 1;
    const bool dense = tier != 1 || (mode != 2 && (A->cf.ndense > 0 || A->ball_limits));
    for (const UhcStepInstance& s : g_steps)
        if (s.queue == queue && s.tier == tier && s.mode == mode && s.dense == dense) return s.launch(A, d_action, d_tbase, d_active, lds_bytes, stream);
    return hipErrorInvalidDeviceFunction;  // (a missing instantiation is an error)
}
static hipError_t uhc_set_lds_limit(size_t lds_bytes, size_t lds_bytes_fast, size_t lds_bytes_big) {
    const size_t bytes[3] = {lds_bytes, lds_bytes_fast, lds_bytes_big};
    for (const UhcStepInstance& s : g_steps) {
        if (s.lds == 2 && !lds_bytes_big) continue;  // (no large tier in this batch)
        const hipError_t e = s.set_lds(bytes[s.lds]);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
extern "C" hipError_t uhc_launch_tier_lists(const int* tier, const int* d_active, int n_env, int* tier_now, int* lists, int* counts, int* cursors, int* fin,
                                            const int* cost, const int* fresh, int* order, int launch4, int* pend3, hipStream_t stream);
extern "C" hipError_t uhc_launch_gate(const int* started, int want, int* waited, long long* trace, hipStream_t stream);
extern "C" hipError_t uhc_launch_set_state(const DevState* s, int nq, int nv, int nu, const int* env_ids, int n,
                                           const double* qpos, const double* qvel, int* mask, hipStream_t stream);

static thread_local std::string g_err;
static int fail(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}
#define HIP_OK(expr)                                                                      \
    do {                                                                                  \
        hipError_t e__ = (expr);                                                          \
        if (e__ != hipSuccess) return fail("%s: %s", #expr, hipGetErrorString(e__));      \
    } while (0)

extern "C" const char* uhc_last_error(void) { return g_err.c_str(); }
extern "C" int32_t uhc_abi_version(void) { return UHC_ABI_VERSION; }
// what kind of build this library is: bit 0 = the solver's measurement switches are compiled in (-DUHC_EXPERIMENTS: UHC_DEBUG bits 8-12 act), bit 1 = stage
// cycle counters (-DUHC_STAGE_PROF), bit 2 = poisoned LDS (-DUHC_POISON_LDS), bit 3 = LDS guard words (-DUHC_GUARD_LDS).  The shipped library returns 0.
extern "C" int32_t uhc_build_flags(void) {
    int32_t f = 0;
#ifdef UHC_EXPERIMENTS
    f |= 1;
#endif
#ifdef UHC_STAGE_PROF
    f |= 2;
#endif
#ifdef UHC_POISON_LDS
    f |= 4;
#endif
#ifdef UHC_GUARD_LDS
    f |= 8;
#endif
    return f;
}

template <class T>
static void take(std::vector<T>& v, const T*& p, size_t n) {
    v.assign(p, p + n);
    if (v.empty()) v.push_back(T());
    p = v.data();
}

extern "C" int32_t uhc_model_create(const UhcModelDesc* in, UhcModel** out) {
    if (!in || !out) return fail("uhc_model_create: null argument");
    if (in->nbody < 1 || in->nbody > UHC_WAVE) return fail("uhc_model_create: nbody=%d outside [1,64]", in->nbody);
    if (in->nv < 1 || in->nv > 2 * UHC_WAVE) return fail("uhc_model_create: nv=%d outside [1,128]", in->nv);
    if (in->njnt > 2 * UHC_WAVE) return fail("uhc_model_create: njnt=%d > 128", in->njnt);
    UhcModel* m = new UhcModel();
    m->d = *in;
    UhcModelDesc& d = m->d;
    const size_t nb = d.nbody, nj = d.njnt, nv = d.nv, ng = d.ngeom;
    take(m->body_parentid, d.body_parentid, nb); take(m->body_jntadr, d.body_jntadr, nb);
    take(m->body_jntnum, d.body_jntnum, nb); take(m->body_dofadr, d.body_dofadr, nb); take(m->body_dofnum, d.body_dofnum, nb);
    take(m->body_pos, d.body_pos, 3 * nb); take(m->body_quat, d.body_quat, 4 * nb); take(m->body_ipos, d.body_ipos, 3 * nb);
    take(m->body_iquat, d.body_iquat, 4 * nb); take(m->body_mass, d.body_mass, nb); take(m->body_inertia, d.body_inertia, 3 * nb);
    take(m->body_invweight0, d.body_invweight0, 2 * nb);
    take(m->jnt_type, d.jnt_type, nj); take(m->jnt_bodyid, d.jnt_bodyid, nj); take(m->jnt_qposadr, d.jnt_qposadr, nj);
    take(m->jnt_dofadr, d.jnt_dofadr, nj); take(m->jnt_limited, d.jnt_limited, nj);
    take(m->jnt_pos, d.jnt_pos, 3 * nj); take(m->jnt_axis, d.jnt_axis, 3 * nj); take(m->jnt_range, d.jnt_range, 2 * nj);
    take(m->jnt_stiffness, d.jnt_stiffness, nj); take(m->jnt_margin, d.jnt_margin, nj);
    take(m->qpos0, d.qpos0, d.nq); take(m->qpos_spring, d.qpos_spring, d.nq);
    take(m->dof_bodyid, d.dof_bodyid, nv); take(m->dof_jntid, d.dof_jntid, nv); take(m->dof_parentid, d.dof_parentid, nv);
    take(m->dof_madr, d.dof_madr, nv + 1);
    take(m->dof_armature, d.dof_armature, nv); take(m->dof_damping, d.dof_damping, nv);
    take(m->dof_frictionloss, d.dof_frictionloss, nv); take(m->dof_invweight0, d.dof_invweight0, nv);
    take(m->geom_type, d.geom_type, ng); take(m->geom_bodyid, d.geom_bodyid, ng); take(m->geom_contype, d.geom_contype, ng);
    take(m->geom_conaffinity, d.geom_conaffinity, ng); take(m->geom_condim, d.geom_condim, ng);
    take(m->geom_vertadr, d.geom_vertadr, ng); take(m->geom_vertnum, d.geom_vertnum, ng);
    take(m->geom_pos, d.geom_pos, 3 * ng); take(m->geom_quat, d.geom_quat, 4 * ng); take(m->geom_size, d.geom_size, 3 * ng);
    take(m->geom_friction, d.geom_friction, 3 * ng); take(m->geom_margin, d.geom_margin, ng); take(m->geom_gap, d.geom_gap, ng);
    take(m->geom_solref, d.geom_solref, 2 * ng); take(m->geom_solimp, d.geom_solimp, 5 * ng);
    take(m->geom_rbound, d.geom_rbound, ng); take(m->geom_center, d.geom_center, 3 * ng);
    take(m->mesh_vert, d.mesh_vert, 3 * (size_t)d.nmeshvert);
    take(m->mesh_adjadr, d.mesh_adjadr, (size_t)d.nmeshvert + 1); take(m->mesh_adj, d.mesh_adj, d.nmeshadj);
    take(m->exclude_pair, d.exclude_pair, 2 * (size_t)d.nexclude);
    take(m->actuator_dofid, d.actuator_dofid, d.nu); take(m->actuator_gear, d.actuator_gear, 3 * (size_t)d.nu);
    // structural checks the kernels rely on
    for (size_t b = 1; b < nb; b++)
        if (d.body_parentid[b] >= (int)b) { delete m; return fail("uhc_model_create: bodies must be in depth-first order"); }
    for (size_t i = 0; i < nv; i++)
        if (d.dof_parentid[i] >= (int)i) { delete m; return fail("uhc_model_create: dofs must be in depth-first order"); }
    *out = m;
    return 0;
}
extern "C" void uhc_model_free(UhcModel* m) { delete m; }
extern "C" int32_t uhc_model_nM(const UhcModel* m) { return m ? m->d.dof_madr[m->d.nv] : -1; }

// ------------------------------------------------------------------ batch
template <class T>
static int upload(UhcBatch* b, const std::vector<T>& h, const T** dptr) {
    void* p = nullptr;
    size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(T);
    HIP_OK(hipMalloc(&p, bytes));
    b->allocs.push_back(p);
    if (!h.empty()) HIP_OK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *dptr = (const T*)p;
    return 0;
}
// UHC_GUARD_LDS=1 (debug, with the guard words in LDS): every zero-initialised device array of a batch -- the state the kernels WRITE -- sits between two
// 256-byte fences of 0xA5; uhc_batch_free checks them ("uhc guard: ... HBM ...")
template <class T>
static int dalloc(UhcBatch* b, size_t n, T** dptr) {
    void* p = nullptr;
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    if (b->hbm_guard) {
        HIP_OK(hipMalloc(&p, bytes + 512));
        HIP_OK(hipMemset(p, 0xA5, bytes + 512));
        HIP_OK(hipMemset((char*)p + 256, 0, bytes));
        b->allocs.push_back(p);
        b->fences.push_back({(char*)p, bytes});
        *dptr = (T*)((char*)p + 256);
        return 0;
    }
    HIP_OK(hipMalloc(&p, bytes));
    HIP_OK(hipMemset(p, 0, bytes));
    b->allocs.push_back(p);
    *dptr = (T*)p;
    return 0;
}
#define TRY(x) do { if (x) return 1; } while (0)


// the topology tables, model blobs, controller gains and schedules of the plan -> device memory (pointers into b->A)
static int upload_plan(UhcBatch* b, const BatchPlan& P, const UhcModelDesc& d, const UhcCtrlDesc* ctrl, const int32_t* h_env_model) {
    KernelArgs& A = b->A;
    DevTopo& T = A.t;
    const int nb = d.nbody, nv = d.nv, nj = d.njnt, ng = d.ngeom;
    auto ivec = [](const int32_t* p, size_t n) { return std::vector<int>(p, p + n); };
    TRY(upload(b, ivec(d.body_parentid, nb), &T.body_parentid)); TRY(upload(b, ivec(d.body_jntadr, nb), &T.body_jntadr));
    TRY(upload(b, ivec(d.body_jntnum, nb), &T.body_jntnum)); TRY(upload(b, ivec(d.body_dofadr, nb), &T.body_dofadr));
    TRY(upload(b, ivec(d.body_dofnum, nb), &T.body_dofnum)); TRY(upload(b, P.body_rootid, &T.body_rootid));
    TRY(upload(b, P.body_nsub, &T.body_nsub)); TRY(upload(b, P.body_lastdof, &T.body_lastdof)); TRY(upload(b, P.body_depth, &T.body_depth));
    TRY(upload(b, ivec(d.jnt_type, nj), &T.jnt_type)); TRY(upload(b, ivec(d.jnt_bodyid, nj), &T.jnt_bodyid));
    TRY(upload(b, ivec(d.jnt_qposadr, nj), &T.jnt_qposadr)); TRY(upload(b, ivec(d.jnt_dofadr, nj), &T.jnt_dofadr));
    TRY(upload(b, ivec(d.jnt_limited, nj), &T.jnt_limited));
    TRY(upload(b, ivec(d.dof_bodyid, nv), &T.dof_bodyid)); TRY(upload(b, ivec(d.dof_jntid, nv), &T.dof_jntid));
    TRY(upload(b, ivec(d.dof_parentid, nv), &T.dof_parentid)); TRY(upload(b, ivec(d.dof_madr, nv + 1), &T.dof_madr));
    TRY(upload(b, P.dof_depth, &T.dof_depth)); TRY(upload(b, P.dof_ndesc, &T.dof_ndesc));
    TRY(upload(b, P.dof_anc, &T.dof_anc)); TRY(upload(b, P.ncommon, &T.dof_ncommon)); TRY(upload(b, P.m_row, &T.m_row)); TRY(upload(b, P.m_col, &T.m_col)); TRY(upload(b, P.m_ij, &T.m_ij));
    TRY(upload(b, ivec(d.geom_type, ng), &T.geom_type)); TRY(upload(b, ivec(d.geom_bodyid, ng), &T.geom_bodyid));
    TRY(upload(b, ivec(d.geom_condim, ng), &T.geom_condim)); TRY(upload(b, ivec(d.geom_vertadr, ng), &T.geom_vertadr));
    TRY(upload(b, ivec(d.geom_vertnum, ng), &T.geom_vertnum));
    TRY(upload(b, P.pg1, &T.pair_g1)); TRY(upload(b, P.pg2, &T.pair_g2));
    TRY(upload(b, P.cg1, &T.cpair_g1)); TRY(upload(b, P.cg2, &T.cpair_g2)); TRY(upload(b, P.dof_rootid, &T.dof_rootid));
    TRY(upload(b, ivec(d.actuator_dofid, d.nu), &T.actuator_dofid));
    TRY(upload(b, P.model_blob, &A.s.model_blob));
    if (h_env_model) TRY(upload(b, std::vector<int>(h_env_model, h_env_model + b->n_env), &A.s.env_model));
    else if (b->n_models > 1) TRY(upload(b, std::vector<int>(b->n_env, 0), &A.s.env_model));  // selectable later (uhc_env_set_clip_models)
    if (A.c.rfc_mode == 2) TRY(upload(b, P.vf_body, &A.c.vf_body));
    auto dvec = [&](const double* p) { return std::vector<double>(p, p + d.nu); };
    TRY(upload(b, dvec(ctrl->jkp), &A.c.jkp)); TRY(upload(b, dvec(ctrl->jkd), &A.c.jkd));
    TRY(upload(b, dvec(ctrl->torque_lim), &A.c.torque_lim)); TRY(upload(b, dvec(ctrl->a_scale), &A.c.a_scale));
    if (!P.guard_tab.empty()) {  // UHC_GUARD_LDS
        const std::vector<int>& tab = P.guard_tab;
        int* d_tab = nullptr;
        TRY(dalloc(b, tab.size(), &d_tab)); TRY(dalloc(b, 4, &b->d_guard_hits));
        HIP_OK(hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
        HIP_OK(hipMemset(b->d_guard_hits, 0, 4 * sizeof(int)));
        A.guard_tab = d_tab; A.guard_hits = b->d_guard_hits;
        fprintf(stderr, "uhc guard: LDS guard words on -- fast %d + %d, general %d + %d, large %d + %d, tier 4 %d + %d (persistent + constraint phase)\n", tab[0], tab[1],
                tab[64], tab[65], tab[128], tab[129], tab[192], tab[193]);
    }
    TRY(upload(b, P.chain, &T.chain));
    TRY(upload(b, P.dof_act, &T.dof_act));
    TRY(upload(b, P.fac_prog, &T.fac_prog)); TRY(upload(b, P.sol_back, &T.sol_back)); TRY(upload(b, P.sol_fwd, &T.sol_fwd));
    return 0;
}

// the per-env state the kernels write (zero-initialised; every env starts in the fast tier at its model's qpos0), and the field table over it
static int alloc_state(UhcBatch* b, const UhcModel* const* models, const int32_t* h_env_model) {
    KernelArgs& A = b->A;
    DevState& S = A.s;
    const size_t E = b->n_env;
    const int nq = A.t.nq, nv = A.t.nv, nu = A.t.nu, nb = A.t.nbody;
    TRY(dalloc(b, E * nq, &S.qpos)); TRY(dalloc(b, E * nv, &S.qvel)); TRY(dalloc(b, E * nv, &S.qacc)); TRY(dalloc(b, E * nv, &S.qacc_ws));
    TRY(dalloc(b, E * 3 * nb, &S.xpos)); TRY(dalloc(b, E * 4 * nb, &S.xquat)); TRY(dalloc(b, E * 3 * nb, &S.xipos));
    TRY(dalloc(b, 4, &S.path_stats));
    TRY(dalloc(b, E * A.t.nM, &S.qM)); TRY(dalloc(b, 6 * E + 1, &S.redo)); S.pend2 = S.redo + E; S.pend3 = S.redo + 2 * E; S.resume = S.redo + 3 * E; S.why = S.redo + 4 * E; TRY(dalloc(b, 2, &S.q_abort));
    A.chunk_done = S.redo + 5 * E; A.ticket = S.redo + 6 * E; TRY(dalloc(b, E * UHC_CHUNK_REC, &A.chunk_rec));  // (the chunked fast tier: progress words and ticket counter are reset with redo .. why)
    TRY(dalloc(b, E, &S.tier)); TRY(dalloc(b, E, &b->tier_now)); S.tier_now = b->tier_now; TRY(dalloc(b, E, &S.cost));
    if (!(A.dbg & 8)) TRY(dalloc(b, E, &b->d_order));  // (UHC_DEBUG bit 3: the fast tier launches in env order)
    TRY(dalloc(b, 3 * E, &b->d_lists)); TRY(dalloc(b, 8, &b->d_counts)); TRY(dalloc(b, 8, &b->d_cursors)); TRY(dalloc(b, 8, &b->d_fin));
    { std::vector<int> one(E, 1); HIP_OK(hipMemcpy(S.tier, one.data(), E * sizeof(int), hipMemcpyHostToDevice)); } TRY(dalloc(b, E, &S.fresh)); TRY(dalloc(b, E * 40, &S.prof)); TRY(dalloc(b, E * nv, &S.bias)); TRY(dalloc(b, E * nu, &S.ctrl));
    TRY(dalloc(b, E * nv, &S.applied));
    if (A.c.rfc_mode == 2) { TRY(dalloc(b, E * 6 * nv, &S.cdof)); TRY(dalloc(b, E * 3 * nb, &S.rootcom)); }
    TRY(dalloc(b, E, &S.ncon)); TRY(dalloc(b, E, &S.nefc)); TRY(dalloc(b, E, &S.fail)); TRY(dalloc(b, E, &S.solver_iter));
    TRY(dalloc(b, E, &S.overflow));
    if (A.last_tier == 4) { TRY(dalloc(b, E * (size_t)A.gy_stride, &A.gY)); TRY(dalloc(b, E * (size_t)A.gd_stride, &A.gD)); }
    TRY(dalloc(b, E, &b->reset_mask));
    // qpos <- qpos0 of each env's model
    {
        std::vector<double> q0(E * nq);
        for (size_t e = 0; e < E; e++) {
            const UhcModelDesc& md = models[h_env_model ? h_env_model[e] : 0]->d;
            memcpy(&q0[e * nq], md.qpos0, nq * sizeof(double));
        }
        HIP_OK(hipMemcpy(S.qpos, q0.data(), q0.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    const int64_t n = (int64_t)E;
    const UhcBatch::Field fields[21] = {{S.qpos, n * nq}, {S.qvel, n * nv}, {S.xpos, n * 3 * nb}, {S.xquat, n * 4 * nb}, {S.xipos, n * 3 * nb}, {S.qM, n * A.t.nM}, {S.bias, n * nv},
                                        {S.qacc, n * nv}, {S.ctrl, n * nu}, {S.ncon, n}, {S.nefc, n}, {S.fail, n}, {S.solver_iter, n}, {S.applied, n * nv}, {S.overflow, n},
                                        {S.prof, n * 40}, {S.redo, n}, {S.tier, n}, {S.why, n}, {S.qacc_ws, n * nv}, {S.cost, n}};
    std::copy(fields, fields + 21, b->field);
    return 0;
}

extern "C" void uhc_batch_free(UhcBatch* b);
// knobs and plan first (every refusal that does not need the device), then the device: from its first allocation the batch is owned by a
// handle that frees it, so no exit leaks device memory
extern "C" int32_t uhc_batch_create(const UhcModel* const* models, int32_t n_models, const int32_t* h_env_model, int32_t n_env,
                                    int32_t device_id, const UhcCtrlDesc* ctrl, UhcBatch** out) {
    if (!out) return fail("uhc_batch_create: bad argument");
    const BatchKnobs knobs = read_knobs();
    BatchPlan P;
    std::string err;
    if (plan_batch(models, n_models, h_env_model, n_env, ctrl, knobs, &P, &err)) return fail("%s", err.c_str());
    int ndev = 0;
    HIP_OK(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail("uhc_batch_create: device %d not present (%d devices)", device_id, ndev);
    HIP_OK(hipSetDevice(device_id));

    std::unique_ptr<UhcBatch, void (*)(UhcBatch*)> owner(new UhcBatch(), uhc_batch_free);
    UhcBatch* b = owner.get();
    b->n_env = n_env;
    b->device = device_id;
    b->n_models = n_models;
    b->n_trailing_free = P.n_trailing_free;
    b->A = P.A;
    b->nM = P.A.t.nM;
    b->lds_bytes = P.lds_bytes; b->lds_bytes_fast = P.lds_bytes_fast; b->lds_bytes_big = P.lds_bytes_big;
    b->use_fast = P.use_fast;
    b->hbm_guard = knobs.guard != 0;
    b->q2_div = knobs.q2_div; b->q2_wait_min = knobs.q2_wait_min; b->q2_max = knobs.q2_max; b->q3_max = knobs.q3_max; b->q4_max = knobs.q4_max;
    b->fast_chunk = (P.A.dbg & 4) ? 0x7fff : knobs.fast_chunk;  // (UHC_DEBUG bit 2 restarts a handed-on env's step from substep 0: only the whole-step launch can)
    TRY(upload_plan(b, P, models[0]->d, ctrl, h_env_model));
    HIP_OK(uhc_set_lds_limit(b->lds_bytes, b->lds_bytes_fast, b->lds_bytes_big));
    TRY(alloc_state(b, models, h_env_model));
    HIP_OK(hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking));
    b->stream = b->own_stream;
    *out = owner.release();
    return 0;
}

static void guard_report(UhcBatch* b) {  // UHC_GUARD_LDS=1: what the kernels found (once per new finding)
    if (!b->d_guard_hits) return;
    int h[4] = {0, 0, 0, 0};
    if (hipMemcpy(h, b->d_guard_hits, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return;
    if (h[0] > b->guard_reported) {
        b->guard_reported = h[0];
        fprintf(stderr, "uhc guard: %d LDS guard words OVERWRITTEN so far; the first: tier %d, %s region %d (offset %d doubles), env %d\n", h[0], h[1] >> 16,
                ((h[1] >> 8) & 0xff) ? "constraint-phase" : "persistent", h[1] & 0xff, h[3], h[2]);
    }
}
extern "C" void uhc_batch_free(UhcBatch* b) {
    if (!b) return;
    hipSetDevice(b->device);
    hipDeviceSynchronize();
    guard_report(b);
    if (!b->fences.empty()) {
        int bad = 0;
        unsigned char h[512];
        for (size_t k = 0; k < b->fences.size(); k++) {
            const auto& f = b->fences[k];
            bool hit = false;
            if (hipMemcpy(h, f.first, 256, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(h + 256, f.first + 256 + f.second, 256, hipMemcpyDeviceToHost) != hipSuccess) continue;
            for (int i = 0; i < 512; i++) hit = hit || h[i] != 0xA5;
            if (hit) { if (!bad) fprintf(stderr, "uhc guard: HBM array %zu (%zu bytes) has an OVERWRITTEN fence\n", k, f.second); bad++; }
        }
        fprintf(stderr, "uhc guard: %zu fenced HBM arrays checked, %d with an overwritten fence\n", b->fences.size(), bad);
    }
    if (b->d_guard_hits) fprintf(stderr, "uhc guard: batch of %d envs freed, %d guard words overwritten in its lifetime\n", b->n_env, b->guard_reported);
    for (void* p : b->allocs) hipFree(p);
    for (auto& ev : b->ev_used) { hipEventDestroy(ev.first); hipEventDestroy(ev.second); }
    for (auto& ev : b->ev_free) { hipEventDestroy(ev.first); hipEventDestroy(ev.second); }
    for (hipEvent_t e : {b->ev_fork, b->ev_side1, b->ev_side2, b->ev_side3}) if (e) hipEventDestroy(e);
    for (hipEvent_t e : b->cnt_ev) if (e) hipEventDestroy(e);
    if (b->h_counts) hipHostFree(b->h_counts);
    if (b->side_stream) hipStreamDestroy(b->side_stream);
    if (b->side_stream3) hipStreamDestroy(b->side_stream3);
    if (b->side_stream4) hipStreamDestroy(b->side_stream4);
    if (b->own_stream) hipStreamDestroy(b->own_stream);
    delete b;
}
extern "C" int32_t uhc_batch_set_stream(UhcBatch* b, void* s) {
    if (!b) return fail("uhc_batch_set_stream: null batch");
    b->stream = (hipStream_t)s;  // NULL is the device's null (default) stream
    return 0;
}
extern "C" int32_t uhc_batch_sync(UhcBatch* b) {
    if (!b) return fail("uhc_batch_sync: null batch");
    HIP_OK(hipStreamSynchronize(b->stream));
    guard_report(b);
    return 0;
}
extern "C" int32_t uhc_batch_set_rfc_scale(UhcBatch* b, double s) {
    if (!b) return fail("uhc_batch_set_rfc_scale: null batch");
    b->A.c.rfc_scale = s;
    return 0;
}
extern "C" int32_t uhc_batch_set_kernel_path(UhcBatch* b, int32_t mode) {
    if (!b) return fail("uhc_batch_set_kernel_path: null batch");
    if (mode < 0 || mode > 2) return fail("uhc_batch_set_kernel_path: mode %d (0 fast then general, 1 general only, 2 adaptive)", mode);
    b->general_only = mode == 1;
    b->path_mode = mode;
    if (mode == 2 && !b->side_stream) {
        HIP_OK(hipSetDevice(b->device));
        // The consumers WAIT for launches of the batch's own stream, so they must never sit behind them in one hardware queue (streams beyond
        // the runtime's pool of hardware queues share one and then run in order).  Streams of another priority get their queues from
        // another pool.  The two side streams may still share a queue with each other: the general tier's consumers are launched first,
        // the large tier's (which wait for them) second, so that in-order execution is merely slower.
        int least = 0, greatest = 0;
        HIP_OK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_OK(hipStreamCreateWithPriority(&b->side_stream, hipStreamNonBlocking, greatest));
        // (the large tier's stream at the LOWEST priority when the device has three levels: a pool of its own, so that its consumers can be
        //  launched BEFORE the general tier's -- they need whole CUs, which they only find while nothing else is resident -- without ever
        //  sharing a queue with the launch they wait for)
        HIP_OK(hipStreamCreateWithPriority(&b->side_stream3, hipStreamNonBlocking, (least != greatest && least != 0) ? least : greatest));
        b->large_first = least != greatest && least != 0;
        { hipDeviceProp_t pr; HIP_OK(hipGetDeviceProperties(&pr, b->device)); b->n_cu = pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256; }
        HIP_OK(hipHostMalloc((void**)&b->h_counts, sizeof(int) * 8 * 8, hipHostMallocDefault));
        memset(b->h_counts, 0, sizeof(int) * 8 * 8);
        for (int k = 0; k < 8; k++) HIP_OK(hipEventCreateWithFlags(&b->cnt_ev[k], hipEventDisableTiming));
        HIP_OK(hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming));
        HIP_OK(hipEventCreateWithFlags(&b->ev_side1, hipEventDisableTiming));
        HIP_OK(hipEventCreateWithFlags(&b->ev_side2, hipEventDisableTiming));
        // tier 4's own launch (envs whose last step ended there): whole CUs, like the large tier's -- same priority class, launched first of all
        HIP_OK(hipStreamCreateWithPriority(&b->side_stream4, hipStreamNonBlocking, (least != greatest && least != 0) ? least : greatest));
        HIP_OK(hipEventCreateWithFlags(&b->ev_side3, hipEventDisableTiming));
    }
    return 0;
}
extern "C" int32_t uhc_batch_set_solver(UhcBatch* b, int32_t solver, int32_t iterations) {
    if (!b || (solver != 0 && solver != 1)) return fail("uhc_batch_set_solver: solver must be 0 (sweeps) or 1 (active set)");
    b->A.t.solver = solver;
    if (iterations > 0) b->A.t.iterations = iterations;
    return 0;
}
extern "C" int32_t uhc_batch_field(UhcBatch* b, int32_t f, void** p, int64_t* n) {
    if (!b || f < 0 || f > 20 || !b->field[f].ptr) return fail("uhc_batch_field: unknown field %d", f);
    if (p) *p = b->field[f].ptr;
    if (n) *n = b->field[f].count;
    return 0;
}
// sticky tiers: an env starts in the tier that computed its last step.  The general / large tiers' own envs run on a side stream
// BESIDE the fast tier (their launches last several times longer per env; in a chain behind it the step would wait for them);
// only the envs a tier hands on this very step go through the chain.  All launches filter on one snapshot of the tier table.
// The sizes of the consumer launches come from the newest queue counts the host has seen: plan_sticky_step (uhc_plan.cpp).
static int launch_sticky(UhcBatch* b, int mode, const double* d_action, const double* d_tbase, const int* d_active, bool timed, std::pair<hipEvent_t, hipEvent_t> ev) {
    const bool big = b->A.last_tier >= 3;
        KernelArgs K = b->A;
        // tier 4's own consumers: when the newest counts seen say that envs went through tier 4 (counts[7]: hand-ons of the large tier + envs that start there),
        // a few persistent workgroups wait on a queue of their own (d_lists + 2 n_env) beside everything else, and the large tier's consumers append what
        // they find too big instead of leaving it for the chained launch at the very end of the step -- where a 10 ms env-step of one env used to be added
        // to every step in which any env needed tier 4 (configs[4]: 64 k -> 42 k env-steps/s when tier 4 came in).  Envs that START in tier 4
        // (UHC_DEBUG bit 12) are put at the head of that queue by the list kernel.
        int est4 = 0, est2_then = 0;
        if (b->A.last_tier == 4 && b->q4_max > 0)
            for (long long k = b->cnt_step - 1; k >= 0 && k > b->cnt_step - 8; k--)
                if (hipEventQuery(b->cnt_ev[k % 8]) == hipSuccess) { est4 = b->h_counts[8 * (k % 8) + 7]; est2_then = b->h_counts[8 * (k % 8) + 2]; break; }
        (void)hipGetLastError();
    StickyInputs in{};
    in.est4 = est4; in.est2_then = est2_then; in.n_env = b->n_env; in.n_cu = b->n_cu; in.lds_bytes_fast = b->lds_bytes_fast; in.large_first = b->large_first;
    in.fast_chunk = b->fast_chunk; in.n_substeps = b->A.c.n_substeps;
    in.last_tier = b->A.last_tier; in.q2_div = b->q2_div; in.q2_wait_min = b->q2_wait_min; in.q2_max = b->q2_max; in.q3_max = b->q3_max; in.q4_max = b->q4_max;
#ifdef UHC_EXPERIMENTS
    in.fixed_cap2 = (b->A.dbg & 2048) != 0;  // (measurement switch: a fixed cap UHC_Q2_MAX on the general tier's consumers)
#endif
    // (the list kernel's view of tier 4's consumers: decided before the back-off bookkeeping below, like the counts it is sized from)
    in.queues_off = b->queues_off;
    const bool launch4 = plan_sticky_step(in).launch4;
        K.cnt4 = b->d_counts + 7;
        HIP_OK(uhc_launch_tier_lists(b->A.s.tier, d_active, b->n_env, b->tier_now, b->d_lists, b->d_counts, b->d_cursors, b->d_fin, b->A.s.cost, b->A.s.fresh, b->d_order,
                                     launch4 ? 1 : 0, b->A.s.pend3, b->stream));
        HIP_OK(hipEventRecord(b->ev_fork, b->stream));
        // how long the queues got is known on the host with a lag (asynchronous copies of the final counts, never waited for): the newest
        // copy that has landed sizes this step's consumer launches.  While the general tier's queue was empty when last seen there are no
        // consumers at all: an env the fast tier hands on is flagged and goes through the chained launches like in mode 0.
        // (the host may not run more than two steps ahead of the device here: a launch sized for a queue of five that meets nine hundred
        //  envs works them off five at a time)
        if (b->cnt_step >= 2) HIP_OK(hipEventSynchronize(b->cnt_ev[(b->cnt_step - 2) % 8]));
        int est2 = 0, est3 = 0, handed2 = 0;  // queue lengths at the end of the newest step seen, and how many of the general tier's came in during the step
        for (long long k = b->cnt_step - 1; k >= 0 && k > b->cnt_step - 8; k--)
            if (hipEventQuery(b->cnt_ev[k % 8]) == hipSuccess) {
                const int* hc = b->h_counts + 8 * (k % 8);
                est2 = hc[2]; est3 = hc[3]; handed2 = std::max(0, hc[2] - hc[4]);
                if (b->A.dbg & 64) fprintf(stderr, "uhc step %lld: queues %d / %d envs (%d handed on), gate waited %.1f us, gave up %d, queues_off %d\n", k, est2, est3, handed2, 0.01 * hc[1], hc[0], (int)b->queues_off);
                if (hc[0] > b->aborts_seen) {  // a consumer gave up waiting: its producers did not run beside it (or too slowly).  No waiting
                    b->aborts_seen = hc[0];     // consumers for the next 32 steps; after the third time, for good
                    b->queues_off_until = ++b->abort_events >= 3 ? (long long)1 << 62 : b->cnt_step + 32;
                }
                b->queues_off = b->cnt_step < b->queues_off_until;
                break;
            }
    in.est2 = est2; in.est3 = est3; in.handed2 = handed2; in.queues_off = b->queues_off;
    const StickySizes z = plan_sticky_step(in);
    const bool queues = z.queues, waiting = z.waiting, q3 = z.q3, q4 = launch4 && q3;
    const int grid2 = z.grid2, grid3 = z.grid3, grid4 = z.grid4;
    K.sticky_mask = (queues ? 4 : 0) | (q3 ? 8 : 0) | (launch4 ? 16 : 0);
        if (q4) {  // (first of the side launches: a whole CU's LDS each, only to be had before the fast tier's launch has filled the chip)
            HIP_OK(hipStreamWaitEvent(b->side_stream4, b->ev_fork, 0));
            K.tier_want = 0; K.list = b->d_lists + 2 * b->n_env; K.list_count = b->d_counts + 6; K.list_cursor = b->d_cursors + 4;
            K.grid = grid4; K.n_wait = grid4; K.spares = nullptr; K.started = nullptr;
            K.prod_fin = b->d_fin + 5; K.prod_total = grid3;  // the large tier's consumers
            K.fin = nullptr; K.q_next = nullptr; K.q_next_count = nullptr;
            if (b->A.dbg & 64) fprintf(stderr, "uhc step %lld: %d tier-4 consumers (%d env-steps went through tier 4 when last seen)\n", b->cnt_step, grid4, est4);
            HIP_OK(uhc_launch_step(mode, 4, &K, d_action, d_tbase, nullptr, b->lds_bytes_big, b->side_stream4));
            HIP_OK(hipEventRecord(b->ev_side3, b->side_stream4));
        }
        auto launch_large = [&]() -> int {
            HIP_OK(hipStreamWaitEvent(b->side_stream3, b->ev_fork, 0));
            K.tier_want = 0; K.list = b->d_lists + b->n_env; K.list_count = b->d_counts + 3; K.list_cursor = b->d_cursors + 3;
            K.grid = grid3; K.n_wait = grid3; K.spares = nullptr; K.started = b->d_fin + 4;
            K.prod_fin = b->d_fin + 2; K.prod_total = grid2;  // the general tier's workgroups: they never wait for this launch
            K.fin = q4 ? b->d_fin + 5 : nullptr; K.q_next = q4 ? b->d_lists + 2 * b->n_env : nullptr; K.q_next_count = q4 ? b->d_counts + 6 : nullptr;
            HIP_OK(uhc_launch_step(mode, 3, &K, d_action, d_tbase, nullptr, b->lds_bytes_big, b->side_stream3));
            HIP_OK(hipEventRecord(b->ev_side2, b->side_stream3));
            return 0;
        };
        // (the large tier's consumers first where their stream has a queue pool of its own: whole CUs are only free while nothing else is
        //  resident, so the general tier's launch waits behind a gate until they have reported in)
        if (q3 && b->large_first) { if (launch_large()) return -1; }
        if (queues) {
            HIP_OK(hipStreamWaitEvent(b->side_stream, b->ev_fork, 0));
            if (q3 && b->large_first && !(b->A.dbg & 32)) HIP_OK(uhc_launch_gate(b->d_fin + 4, grid3, nullptr, nullptr, b->side_stream));
            K.tier_want = 0; K.list = b->d_lists; K.list_count = b->d_counts + 2; K.list_cursor = b->d_cursors + 2;
            K.grid = grid2;
            K.prod_fin = waiting ? b->d_fin + 1 : nullptr; K.prod_total = z.fast.prod_total;  // every workgroup of the fast tier's launch below
            K.fin = b->d_fin + 2; K.started = waiting ? b->d_fin + 3 : nullptr;
            K.n_wait = z.n_wait; K.spares = b->d_fin;
            K.q_next = q3 ? b->d_lists + b->n_env : nullptr; K.q_next_count = q3 ? b->d_counts + 3 : nullptr;
            HIP_OK(uhc_launch_step(mode, 2, &K, d_action, d_tbase, nullptr, b->lds_bytes, b->side_stream));
            HIP_OK(hipEventRecord(b->ev_side1, b->side_stream));
        }
        if (q3 && !b->large_first) { if (launch_large()) return -1; }
        K.list = nullptr; K.list_count = nullptr; K.list_cursor = nullptr; K.grid = 0; K.prod_fin = nullptr; K.prod_total = 0; K.started = nullptr; K.spares = nullptr;
        // The fast tier's launch fills every CU's LDS the moment it starts; consumers that are not resident by then get theirs only when
        // its first workgroups leave (the tier trace showed them starting 3.7 ms into the step).  A one-thread gate on this stream holds
        // the launch back until every consumer workgroup has reported in (or 200 us have passed).
        if (waiting && !(b->A.dbg & 32)) HIP_OK(uhc_launch_gate(b->d_fin + 3, grid2, b->d_counts + 1,
                                                                     (b->A.dbg & 16) ? b->A.s.prof + (size_t)(b->n_env - 1) * 40 + 16 : nullptr, b->stream));
        K.tier_want = 1;
        K.chunk = z.fast.chunk; K.grid = z.fast.chunk ? z.fast.grid : 0;  // (in substep chunks: n_chunks x n_env workgroups, chunk-major by ticket)
        K.order = b->d_order;  // (costliest envs first; null with UHC_DEBUG bit 3: env order)
        K.fin = waiting ? b->d_fin + 1 : nullptr;
        K.q_next = waiting ? b->d_lists : nullptr; K.q_next_count = waiting ? b->d_counts + 2 : nullptr;
        if (timed) HIP_OK(hipEventRecord(ev.first, b->stream));
        HIP_OK(uhc_launch_step(mode, 1, &K, d_action, d_tbase, d_active, b->lds_bytes_fast, b->stream));
        if (timed) { HIP_OK(hipEventRecord(ev.second, b->stream)); b->ev_used.push_back(ev); }
        K.tier_want = 0; K.sticky_mask = 0; K.fin = nullptr; K.q_next = nullptr; K.q_next_count = nullptr; K.order = nullptr; K.chunk = 0; K.grid = 0;
        // chained launches on what is still flagged: everything handed on when no consumers run, nothing (two empty launches) when they do
        if (queues) HIP_OK(hipStreamWaitEvent(b->stream, b->ev_side1, 0));
        HIP_OK(uhc_launch_step(mode, 2, &K, d_action, d_tbase, b->A.s.pend2, b->lds_bytes, b->stream));
        if (q3) HIP_OK(hipStreamWaitEvent(b->stream, b->ev_side2, 0));
        if (q4) HIP_OK(hipStreamWaitEvent(b->stream, b->ev_side3, 0));
        if (big) HIP_OK(uhc_launch_step(mode, 3, &K, d_action, d_tbase, b->A.s.pend3, b->lds_bytes_big, b->stream));
        // the final queue lengths of this step, for the steps to come
        const int slot = (int)(b->cnt_step % 8);
        HIP_OK(hipMemcpyAsync(b->d_counts, b->A.s.q_abort, sizeof(int), hipMemcpyDeviceToDevice, b->stream));  // counts[0] carries the give-up count
        HIP_OK(hipMemcpyAsync(b->h_counts + 8 * slot, b->d_counts, 8 * sizeof(int), hipMemcpyDeviceToHost, b->stream));
        HIP_OK(hipEventRecord(b->cnt_ev[slot], b->stream));
        b->cnt_step++;
        return 0;
    }

// fast kernel on every (active) env, then the general kernel on the envs that raised redo
static int launch(UhcBatch* b, int mode, const double* d_action, const double* d_tbase, const int* d_active) {
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    const bool timed = b->timing && mode == 0;  // HIP events around the kernel that does the work of a control step
    if (timed) {
        if (b->ev_free.empty()) { HIP_OK(hipEventCreate(&ev.first)); HIP_OK(hipEventCreate(&ev.second)); }
        else { ev = b->ev_free.back(); b->ev_free.pop_back(); }
    }
    const bool general = b->general_only;
    const bool big = b->A.last_tier >= 3;  // (tier 4 has no chained launch of its own: the large tier's workgroups go on with it; under sticky tiers it has queue consumers)
    // tier chain: every tier works on the envs the previous one flagged (redo / redo2) and left untouched
    HIP_OK(hipMemsetAsync(b->A.s.redo, 0, sizeof(int) * ((size_t)b->n_env * 6 + 1), b->stream));  // redo (the step's UHC_F_REDO words), pend2, pend3, resume, why, chunk_done, ticket: one allocation
    // (inside a stream capture the sticky launch cannot be used: it sizes its consumer launches from counts the host reads between steps
    //  -- event queries and a wait that are not allowed while capturing, and a replay would repeat the capture step's sizes anyway.  A
    //  captured step takes the plain tier chain, which computes the same step.)
    bool capturing = false;
    {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(b->stream, &cs) == hipSuccess) capturing = cs == hipStreamCaptureStatusActive;
        else (void)hipGetLastError();
    }
    if (mode == 0 && b->path_mode == 2 && b->use_fast && !general && !capturing) return launch_sticky(b, mode, d_action, d_tbase, d_active, timed, ev);
    if (b->use_fast && !general) {
        if (timed) HIP_OK(hipEventRecord(ev.first, b->stream));
        KernelArgs K = b->A;
        if (mode == 0) {  // the control step in substep chunks (the forward-only and kinematics launches have no substeps)
            const FastChunks f = plan_fast_chunks(K.c.n_substeps, default_fast_chunk(b->fast_chunk, K.c.n_substeps, b->n_env, b->n_cu, b->lds_bytes_fast), b->n_env);
            K.chunk = f.chunk; K.grid = f.chunk ? f.grid : 0;
        }
        HIP_OK(uhc_launch_step(mode, 1, &K, d_action, d_tbase, d_active, b->lds_bytes_fast, b->stream));
        if (timed) { HIP_OK(hipEventRecord(ev.second, b->stream)); b->ev_used.push_back(ev); }
        HIP_OK(uhc_launch_step(mode, 2, &b->A, d_action, d_tbase, b->A.s.pend2, b->lds_bytes, b->stream));
    } else {
        if (timed) HIP_OK(hipEventRecord(ev.first, b->stream));
        HIP_OK(uhc_launch_step(mode, 2, &b->A, d_action, d_tbase, d_active, b->lds_bytes, b->stream));
        if (timed) { HIP_OK(hipEventRecord(ev.second, b->stream)); b->ev_used.push_back(ev); }
    }
    if (big) HIP_OK(uhc_launch_step(mode, 3, &b->A, d_action, d_tbase, b->A.s.pend3, b->lds_bytes_big, b->stream));
    return 0;
}

extern "C" int32_t uhc_batch_set_overflow_mode(UhcBatch* b, int32_t truncate) {
    if (!b) return fail("uhc_batch_set_overflow_mode: null batch");
    b->A.truncate = truncate != 0;
    return 0;
}
extern "C" int32_t uhc_batch_set_timing(UhcBatch* b, int32_t enable) {
    if (!b) return fail("uhc_batch_set_timing: null batch");
    b->timing = enable != 0;
    return 0;
}
extern "C" int32_t uhc_batch_kernel_time(UhcBatch* b, double* total_ms, int32_t* launches) {
    if (!b || !total_ms || !launches) return fail("uhc_batch_kernel_time: null argument");
    double tot = 0;
    for (auto& ev : b->ev_used) {
        float ms = 0;
        HIP_OK(hipEventSynchronize(ev.second));
        HIP_OK(hipEventElapsedTime(&ms, ev.first, ev.second));
        tot += ms;
        b->ev_free.push_back(ev);
    }
    *total_ms = tot;
    *launches = (int32_t)b->ev_used.size();
    b->ev_used.clear();
    return 0;
}

extern "C" int32_t uhc_batch_give_ups(UhcBatch* b, int32_t* n, int32_t* n_slow) {
    if (!b || !n) return fail("uhc_batch_give_ups: null argument");
    HIP_OK(hipSetDevice(b->device));
    HIP_OK(hipStreamSynchronize(b->stream));
    int v[2] = {0, 0};
    HIP_OK(hipMemcpy(v, b->A.s.q_abort, sizeof v, hipMemcpyDeviceToHost));
    *n = v[0];
    if (n_slow) *n_slow = v[1];
    return 0;
}

extern "C" int32_t uhc_batch_forward(UhcBatch* b) {
    if (!b) return fail("uhc_batch_forward: null batch");
    HIP_OK(hipSetDevice(b->device));
    return launch(b, 1, nullptr, nullptr, nullptr);
}
extern "C" int32_t uhc_batch_set_state(UhcBatch* b, const int32_t* d_env_ids, int32_t n, const double* d_qpos, const double* d_qvel) {
    if (!b || !d_qpos || !d_qvel) return fail("uhc_batch_set_state: null argument");
    if (n < 1 || n > b->n_env) return fail("uhc_batch_set_state: n=%d outside [1,%d]", n, b->n_env);
    if (!d_env_ids && n != b->n_env) return fail("uhc_batch_set_state: env_ids==NULL requires n == n_env");
    HIP_OK(hipSetDevice(b->device));
    HIP_OK(hipMemsetAsync(b->reset_mask, 0, sizeof(int) * b->n_env, b->stream));
    HIP_OK(uhc_launch_set_state(&b->A.s, b->A.t.nq, b->A.t.nv, b->A.t.nu, d_env_ids, n, d_qpos, d_qvel, b->reset_mask, b->stream));
    // sim.forward() on the listed envs only (the others keep their one-substep-stale qM / qfrc_bias)
    return launch(b, 1, nullptr, nullptr, b->reset_mask);
}
extern "C" int32_t uhc_batch_simulate(UhcBatch* b, const double* d_action, const double* d_target_base, const int32_t* d_active) {
    if (!b || !d_action || !d_target_base) return fail("uhc_batch_simulate: null argument");
    HIP_OK(hipSetDevice(b->device));
    return launch(b, 0, d_action, d_target_base, d_active);
}

extern "C" hipError_t uhc_launch_set_state_masked(const DevState* s, int nq, int nv, int nu, int n_env, const int* select, const double* qpos,
                                                  const double* qvel, int* mask, hipStream_t stream);
// env layer: set_state + forward on the envs flagged in d_select (rows of d_qpos / d_qvel are indexed by env)
extern "C" int uhc_internal_set_state_masked(UhcBatch* b, const int* d_select, const double* d_qpos, const double* d_qvel) {
    HIP_OK(hipSetDevice(b->device));
    HIP_OK(uhc_launch_set_state_masked(&b->A.s, b->A.t.nq, b->A.t.nv, b->A.t.nu, b->n_env, d_select, d_qpos, d_qvel, b->reset_mask, b->stream));
    // only the kinematics now (the reset observation reads body poses); the dynamics part of sim.forward() runs at the head of the
    // env's next step kernel (DevState::fresh), which saves a forward-pass-long launch per control step
    const bool kf = b->use_fast && !b->general_only;
    HIP_OK(uhc_launch_step(2, kf ? 1 : 2, &b->A, nullptr, nullptr, b->reset_mask, kf ? b->lds_bytes_fast : b->lds_bytes, b->stream));
    return 0;
}

extern "C" int uhc_internal_trailing_free(UhcBatch* b) { return b->n_trailing_free; }
extern "C" int* uhc_internal_env_model(UhcBatch* b, int* n_models) { *n_models = b->n_models; return const_cast<int*>(b->A.s.env_model); }
// ------------------------------------------------------------------ internal accessors for the env layer (uhc_env_capi.cpp)
extern "C" int uhc_internal_set_error(const char* msg) { return fail("%s", msg); }
extern "C" int uhc_internal_batch_info(UhcBatch* b, int* n_env, int* nq, int* nv, int* nu, int* nbody, int* action_dim, int* vf_dim,
                                       double* dt, double* base_rot_inv, void** stream, int** reset_mask) {
    *n_env = b->n_env; *nq = b->A.t.nq; *nv = b->A.t.nv; *nu = b->A.t.nu; *nbody = b->A.t.nbody;
    *action_dim = b->A.c.action_dim; *vf_dim = b->A.c.rfc_mode == 1 ? 6 : b->A.c.rfc_mode == 2 ? b->A.c.n_vf_body * b->A.c.body_vf_dim : 0;
    *dt = b->A.t.timestep * b->A.c.n_substeps;
    for (int k = 0; k < 4; k++) base_rot_inv[k] = b->A.c.base_rot_inv[k];
    *stream = (void*)b->stream;
    *reset_mask = b->reset_mask;
    return 0;
}
