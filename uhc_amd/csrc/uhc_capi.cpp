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

#include "uhc_api_check.h"  // uhc_internal_set_error (defined below), HIP_OK
#include "uhc_env_plan.h"   // UhcBatchInfo
#include "uhc_host.h"
#include "uhc_internal.h"
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
extern "C" const char* uhc_last_error(void) { return g_err.c_str(); }
extern "C" int32_t uhc_abi_version(void) { return UHC_ABI_VERSION; }
// what kind of build this library is: bit 0 = the solver's measurement switches are compiled in (-DUHC_EXPERIMENTS: UHC_DEBUG_EXP_* act), bit 1 = stage
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
    TRY(upload(b, P.dof_anc, &T.dof_anc)); TRY(upload(b, P.chainmask, &T.dof_chainmask)); TRY(upload(b, P.m_row, &T.m_row)); TRY(upload(b, P.m_col, &T.m_col)); TRY(upload(b, P.m_ij, &T.m_ij));
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
    TRY(dalloc(b, E * A.t.nM, &S.qM)); TRY(dalloc(b, 2, &S.q_abort));
    const StepWords W = step_words(E);  // (one allocation: the chunked fast tier's progress words and ticket counter are reset with redo .. why)
    TRY(dalloc(b, W.total, &S.redo)); S.pend2 = S.redo + W.pend2; S.pend3 = S.redo + W.pend3; S.resume = S.redo + W.resume; S.why = S.redo + W.why;
    A.chunk_done = S.redo + W.chunk_done; A.ticket = S.redo + W.ticket; TRY(dalloc(b, E * UHC_CHUNK_REC, &A.chunk_rec));
    TRY(dalloc(b, E, &S.tier)); TRY(dalloc(b, E, &b->tier_now)); S.tier_now = b->tier_now; TRY(dalloc(b, E, &S.cost));
    if (!(A.dbg & UHC_DEBUG_ENV_ORDER)) TRY(dalloc(b, E, &b->d_order));
    TRY(dalloc(b, UHC_N_LISTS * E, &b->d_lists)); TRY(dalloc(b, UHC_N_WORDS, &b->d_counts)); TRY(dalloc(b, UHC_N_WORDS, &b->d_cursors)); TRY(dalloc(b, UHC_N_WORDS, &b->d_fin));
    { std::vector<int> one(E, 1); HIP_OK(hipMemcpy(S.tier, one.data(), E * sizeof(int), hipMemcpyHostToDevice)); } TRY(dalloc(b, E, &S.fresh)); TRY(dalloc(b, E * UHC_NPROF, &S.prof)); TRY(dalloc(b, E * nv, &S.bias)); TRY(dalloc(b, E * nu, &S.ctrl));
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
    const UhcBatch::Field fields[UHC_F_COST + 1] = {{S.qpos, n * nq}, {S.qvel, n * nv}, {S.xpos, n * 3 * nb}, {S.xquat, n * 4 * nb}, {S.xipos, n * 3 * nb}, {S.qM, n * A.t.nM}, {S.bias, n * nv},
                                        {S.qacc, n * nv}, {S.ctrl, n * nu}, {S.ncon, n}, {S.nefc, n}, {S.fail, n}, {S.solver_iter, n}, {S.applied, n * nv}, {S.overflow, n},
                                        {S.prof, n * UHC_NPROF}, {S.redo, n}, {S.tier, n}, {S.why, n}, {S.qacc_ws, n * nv}, {S.cost, n}};
    std::copy(fields, fields + UHC_F_COST + 1, b->field);
    return 0;
}

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
    b->caps = knobs;
    b->fast_chunk = (P.A.dbg & UHC_DEBUG_RESTART_HANDON) ? 0x7fff : knobs.fast_chunk;  // (a handed-on env's step restarts from substep 0: only the whole-step launch can)
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
        HIP_OK(hipHostMalloc((void**)&b->h_counts, sizeof(int) * 8 * UHC_N_WORDS, hipHostMallocDefault));
        memset(b->h_counts, 0, sizeof(int) * 8 * UHC_N_WORDS);
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
    if (!b || f < 0 || f > UHC_F_COST || !b->field[f].ptr) return fail("uhc_batch_field: unknown field %d", f);
    if (p) *p = b->field[f].ptr;
    if (n) *n = b->field[f].count;
    return 0;
}
typedef std::pair<hipEvent_t, hipEvent_t> EvPair;
// a launch on the batch's stream between two HIP events when the step is timed (ev != null): "the kernel that does the work" of uhc_batch_kernel_time
static int launch_timed(UhcBatch* b, const EvPair* ev, int mode, int tier, const KernelArgs* K, const double* d_action, const double* d_tbase, const int* d_active, size_t lds_bytes) {
    if (ev) HIP_OK(hipEventRecord(ev->first, b->stream));
    HIP_OK(uhc_launch_step(mode, tier, K, d_action, d_tbase, d_active, lds_bytes, b->stream));
    if (ev) { HIP_OK(hipEventRecord(ev->second, b->stream)); b->ev_used.push_back(*ev); }
    return 0;
}

// sticky tiers: an env starts in the tier that computed its last step.  The general / large tiers' own envs run on a side stream
// BESIDE the fast tier (their launches last several times longer per env; in a chain behind it the step would wait for them);
// only the envs a tier hands on this very step go through the chain.  All launches filter on one snapshot of the tier table.
// Which launches a step has, their sizes and how their queues are wired is decided by plan_sticky_step / sticky_wiring (uhc_plan.cpp) from
// the newest queue counts the host has seen; what follows is the device work.

// How long the queues got is known on the host with a lag (asynchronous copies of the final counts, never waited for): the newest row of
// h_counts that has landed -> its step in *step --, or null while none of the last seven steps' has.
static const int* newest_counts(UhcBatch* b, long long* step) {
    const int* row = nullptr;
    for (long long k = b->cnt_step - 1; k >= 0 && k > b->cnt_step - 8 && !row; k--)
        if (hipEventQuery(b->cnt_ev[k % 8]) == hipSuccess) { row = b->h_counts + UHC_N_WORDS * (k % 8); *step = k; }
    (void)hipGetLastError();  // (a query that says "not ready" is no error of the step)
    return row;
}
// The back-off.  A consumer gave up waiting: its producers did not run beside it (or too slowly).  No waiting consumers for the next 32
// steps; after the third time, for good.
static void update_back_off(UhcBatch* b, int give_ups) {
    if (give_ups > b->aborts_seen) {
        b->aborts_seen = give_ups;
        b->queues_off_until = ++b->abort_events >= 3 ? (long long)1 << 62 : b->cnt_step + 32;
    }
    b->queues_off = b->cnt_step < b->queues_off_until;
}
// the KernelArgs of one entry of the step's table: the batch's, with the entry's slots resolved against the batch's lists / counts / cursors / fin.
// A field the entry does not name is null or zero -- also where the launch before it on the host had it set: n_wait, spares, prod_fin and prod_total are
// read by queue_claim alone and `started` by uhc_step_queue_kernel alone (uhc_physics_impl.h), the kernel of a launch that has a list.
static KernelArgs wire_launch(const UhcBatch* b, const StepLaunch& L, int sticky_mask) {
    auto at = [](int* base, int slot, size_t stride) { return slot == UHC_NONE ? nullptr : base + slot * stride; };
    const size_t E = b->n_env;
    KernelArgs K = b->A;
    K.cnt4 = b->d_counts + UHC_CNT_T4_STEPS;
    K.sticky_mask = sticky_mask;
    K.tier_want = L.tier_want;
    K.list = at(b->d_lists, L.list, E); K.list_count = at(b->d_counts, L.count, 1); K.list_cursor = at(b->d_cursors, L.cursor, 1);
    K.grid = (L.list != UHC_NONE || L.chunk) ? L.grid : 0;  // (0: one workgroup per env, the whole-step launch)
    K.n_wait = L.n_wait; K.spares = at(b->d_fin, L.spares, 1); K.started = at(b->d_fin, L.started, 1);
    K.prod_fin = at(b->d_fin, L.prod_fin, 1); K.prod_total = L.prod_total;
    K.fin = at(b->d_fin, L.fin, 1);
    K.q_next = at(b->d_lists, L.next_list, E); K.q_next_count = at(b->d_counts, L.next_count, 1);
    K.chunk = L.chunk;
    K.order = L.use_order ? b->d_order : nullptr;  // (null with UHC_DEBUG_ENV_ORDER)
    return K;
}
static int launch_sticky(UhcBatch* b, int mode, const double* d_action, const double* d_tbase, const int* d_active, const EvPair* ev) {
    StickyInputs in{};
    in.n_env = b->n_env; in.n_cu = b->n_cu; in.lds_bytes_fast = b->lds_bytes_fast; in.large_first = b->large_first;
    in.fast_chunk = b->fast_chunk; in.n_substeps = b->A.c.n_substeps; in.last_tier = b->A.last_tier; set_caps(in, b->caps);
#ifdef UHC_EXPERIMENTS
    in.fixed_cap2 = (b->A.dbg & UHC_DEBUG_EXP_FIXED_CAP2) != 0;  // (measurement switch: a fixed cap UHC_Q2_MAX on the general tier's consumers)
#endif
    long long seen = 0;
    // tier 4's consumers: the list kernel fills their queue, so this is decided first -- before the back-off bookkeeping below, like the counts it is sized from
    if (b->A.last_tier == 4 && b->caps.q4_max > 0)
        if (const int* hc = newest_counts(b, &seen)) { in.est4 = hc[UHC_CNT_T4_STEPS]; in.est2_then = hc[UHC_CNT_GEN]; }
    const bool launch4 = sticky_launch4(in.last_tier, in.est4, in.est2_then, b->queues_off);
    HIP_OK(uhc_launch_tier_lists(b->A.s.tier, d_active, b->n_env, b->tier_now, b->d_lists, b->d_counts, b->d_cursors, b->d_fin, b->A.s.cost, b->A.s.fresh, b->d_order,
                                 launch4 ? 1 : 0, b->A.s.pend3, b->stream));
    HIP_OK(hipEventRecord(b->ev_fork, b->stream));
    // The newest counts that have landed size this step's consumer launches.  While the general tier's queue was empty when last seen there
    // are no consumers at all: an env the fast tier hands on is flagged and goes through the chained launches like in mode 0.
    // (the host may not run more than two steps ahead of the device here: a launch sized for a queue of five that meets nine hundred
    //  envs works them off five at a time)
    if (b->cnt_step >= 2) HIP_OK(hipEventSynchronize(b->cnt_ev[(b->cnt_step - 2) % 8]));
    if (const int* hc = newest_counts(b, &seen)) {
        // queue lengths at the end of the newest step seen, and how many of the general tier's came in during the step
        in.est2 = hc[UHC_CNT_GEN]; in.est3 = hc[UHC_CNT_BIG]; in.handed2 = std::max(0, hc[UHC_CNT_GEN] - hc[UHC_CNT_GEN_HEAD]);
        if (b->A.dbg & UHC_DEBUG_LOG)
            fprintf(stderr, "uhc step %lld: queues %d / %d envs (%d handed on), gate waited %.1f us, gave up %d, queues_off %d\n", seen, in.est2, in.est3, in.handed2,
                    0.01 * hc[UHC_CNT_GATE_WAIT], hc[UHC_CNT_GIVE_UPS], (int)b->queues_off);
        update_back_off(b, hc[UHC_CNT_GIVE_UPS]);
    }
    in.queues_off = b->queues_off;
    const StickySizes z = plan_sticky_step(in, launch4);
    const StepWiring w = sticky_wiring(z, b->large_first);
    const hipStream_t streams[4] = {b->stream, b->side_stream, b->side_stream3, b->side_stream4};   // by StepStream
    const hipEvent_t joins[4] = {nullptr, b->ev_side1, b->ev_side2, b->ev_side3};                  // a side stream's launch done: the chain waits for it
    const size_t lds[5] = {0, b->lds_bytes_fast, b->lds_bytes, b->lds_bytes_big, b->lds_bytes_big};  // by tier
    for (int k = 0; k < w.n; k++) {
        const StepLaunch& L = w.launch[k];
        const hipStream_t st = streams[L.stream];
        const bool side = L.stream != STREAM_MAIN;
        if (side) HIP_OK(hipStreamWaitEvent(st, b->ev_fork, 0));
        if (L.gate_started != UHC_NONE && !(b->A.dbg & UHC_DEBUG_NO_GATE))  // (under UHC_DEBUG_TRACE: the trace of the gate that reports its wait, in the record of the last env)
            HIP_OK(uhc_launch_gate(b->d_fin + L.gate_started, L.gate_want, L.gate_waited != UHC_NONE ? b->d_counts + L.gate_waited : nullptr,
                                   (L.gate_waited != UHC_NONE && (b->A.dbg & UHC_DEBUG_TRACE)) ? b->A.s.prof + (size_t)(b->n_env - 1) * UHC_NPROF + UHC_TRACE_GATE : nullptr, st));
        if (L.tier == 4 && (b->A.dbg & UHC_DEBUG_LOG)) fprintf(stderr, "uhc step %lld: %d tier-4 consumers (%d env-steps went through tier 4 when last seen)\n", b->cnt_step, L.grid, in.est4);
        const KernelArgs K = wire_launch(b, L, z.sticky_mask);
        if (side) {
            HIP_OK(uhc_launch_step(mode, L.tier, &K, d_action, d_tbase, nullptr, lds[L.tier], st));
            HIP_OK(hipEventRecord(joins[L.stream], st));
        } else TRY(launch_timed(b, ev, mode, L.tier, &K, d_action, d_tbase, d_active, lds[L.tier]));
    }
    // chained launches on what is still flagged: everything handed on when no consumers run, nothing (two empty launches) when they do
    KernelArgs K = b->A;
    K.cnt4 = b->d_counts + UHC_CNT_T4_STEPS;
    if (z.queues) HIP_OK(hipStreamWaitEvent(b->stream, b->ev_side1, 0));
    HIP_OK(uhc_launch_step(mode, 2, &K, d_action, d_tbase, b->A.s.pend2, b->lds_bytes, b->stream));
    if (z.q3) HIP_OK(hipStreamWaitEvent(b->stream, b->ev_side2, 0));
    if (z.q4) HIP_OK(hipStreamWaitEvent(b->stream, b->ev_side3, 0));
    if (b->A.last_tier >= 3) HIP_OK(uhc_launch_step(mode, 3, &K, d_action, d_tbase, b->A.s.pend3, b->lds_bytes_big, b->stream));
    // the final queue lengths of this step, for the steps to come
    const int slot = (int)(b->cnt_step % 8);
    HIP_OK(hipMemcpyAsync(b->d_counts + UHC_CNT_GIVE_UPS, b->A.s.q_abort, sizeof(int), hipMemcpyDeviceToDevice, b->stream));
    HIP_OK(hipMemcpyAsync(b->h_counts + UHC_N_WORDS * slot, b->d_counts, UHC_N_WORDS * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    HIP_OK(hipEventRecord(b->cnt_ev[slot], b->stream));
    b->cnt_step++;
    return 0;
}

// fast kernel on every (active) env, then the general kernel on the envs that raised redo
static int launch(UhcBatch* b, int mode, const double* d_action, const double* d_tbase, const int* d_active) {
    EvPair pair{nullptr, nullptr};
    const bool timed = b->timing && mode == 0;  // HIP events around the kernel that does the work of a control step
    if (timed) {
        if (b->ev_free.empty()) { HIP_OK(hipEventCreate(&pair.first)); HIP_OK(hipEventCreate(&pair.second)); }
        else { pair = b->ev_free.back(); b->ev_free.pop_back(); }
    }
    const EvPair* ev = timed ? &pair : nullptr;
    const bool general = b->general_only;
    const bool big = b->A.last_tier >= 3;  // (tier 4 has no chained launch of its own: the large tier's workgroups go on with it; under sticky tiers it has queue consumers)
    // tier chain: every tier works on the envs the previous one flagged (redo / redo2) and left untouched
    HIP_OK(hipMemsetAsync(b->A.s.redo, 0, sizeof(int) * step_words(b->n_env).total, b->stream));
    // (inside a stream capture the sticky launch cannot be used: it sizes its consumer launches from counts the host reads between steps
    //  -- event queries and a wait that are not allowed while capturing, and a replay would repeat the capture step's sizes anyway.  A
    //  captured step takes the plain tier chain, which computes the same step.)
    bool capturing = false;
    {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(b->stream, &cs) == hipSuccess) capturing = cs == hipStreamCaptureStatusActive;
        else (void)hipGetLastError();
    }
    if (mode == 0 && b->path_mode == 2 && b->use_fast && !general && !capturing) return launch_sticky(b, mode, d_action, d_tbase, d_active, ev);
    if (b->use_fast && !general) {
        KernelArgs K = b->A;
        if (mode == 0) {  // the control step in substep chunks (the forward-only and kinematics launches have no substeps)
            const FastChunks f = plan_fast_chunks(K.c.n_substeps, default_fast_chunk(b->fast_chunk, K.c.n_substeps, b->n_env, b->n_cu, b->lds_bytes_fast), b->n_env);
            K.chunk = f.chunk; K.grid = f.chunk ? f.grid : 0;
        }
        TRY(launch_timed(b, ev, mode, 1, &K, d_action, d_tbase, d_active, b->lds_bytes_fast));
        HIP_OK(uhc_launch_step(mode, 2, &b->A, d_action, d_tbase, b->A.s.pend2, b->lds_bytes, b->stream));
    } else TRY(launch_timed(b, ev, mode, 2, &b->A, d_action, d_tbase, d_active, b->lds_bytes));
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

// ------------------------------------------------------------------ what the env layer (uhc_env_capi.cpp) reads and asks of a batch: uhc_internal.h
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

extern "C" int* uhc_internal_env_model(UhcBatch* b, int* n_models) { *n_models = b->n_models; return const_cast<int*>(b->A.s.env_model); }
extern "C" int uhc_internal_set_error(const char* msg) { return fail("%s", msg); }
extern "C" hipStream_t uhc_internal_stream(UhcBatch* b) { return b->stream; }
extern "C" int* uhc_internal_reset_mask(UhcBatch* b) { return b->reset_mask; }
extern "C" UhcBatchInfo uhc_internal_batch_info(UhcBatch* b) {
    const KernelArgs& A = b->A;
    UhcBatchInfo I = {};
    I.n_env = b->n_env; I.nq = A.t.nq; I.nv = A.t.nv; I.nu = A.t.nu; I.nbody = A.t.nbody;
    I.action_dim = A.c.action_dim; I.vf_dim = A.c.rfc_mode == 1 ? 6 : A.c.rfc_mode == 2 ? A.c.n_vf_body * A.c.body_vf_dim : 0;
    I.dt = A.t.timestep * A.c.n_substeps;
    for (int k = 0; k < 4; k++) I.base_rot_inv[k] = A.c.base_rot_inv[k];
    I.n_trailing_free = b->n_trailing_free;
    return I;
}
