// uhc_env_capi.cpp -- host side of the env layer C-ABI (include/uhc_amd.h, "Env layer").
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/uhc_amd.h"
#include "uhc_api_check.h"  // uhc_internal_set_error, HIP_OK
#include "uhc_device_env.h"
#include "uhc_env_plan.h"     // plan_env: what an env is, decided without the device
#include "uhc_expert_math.h"  // XfTree, LiveState: what uhc_env_live_push hands its kernel
#include "uhc_internal.h"     // the launchers of uhc_env.hip / uhc_live.hip, the batch's accessors

struct UhcEnv {
    UhcBatch* b = nullptr;
    EnvArgs E;
    std::vector<void*> allocs;
    double *stage_qpos = nullptr, *stage_qvel = nullptr;
    int* select = nullptr;
    int n_clips = 0;
    int64_t n_frames = 0;
    LiveState live;  // live targets (uhc_env_live_*)
};
#define NOT_WHILE_LIVE(e, who) \
    if ((e)->live.on) return uhc_internal_set_error(who ": the env is in live mode (uhc_env_live_begin): a stream has no window to assign or queue -- push a restart row and uhc_env_reset, or uhc_env_live_end first")

template <class T>
static int dalloc(UhcEnv* e, size_t n, T** p) {
    void* q = nullptr;
    if (hipMalloc(&q, (n ? n : 1) * sizeof(T)) != hipSuccess) return uhc_internal_set_error("uhc_env: hipMalloc failed");
    e->allocs.push_back(q);
    HIP_OK(hipMemset(q, 0, (n ? n : 1) * sizeof(T)));
    *p = (T*)q;
    return 0;
}
static hipStream_t stream_of(UhcEnv* e) { return uhc_internal_stream(e->b); }  // (per call: uhc_batch_set_stream may have changed it)

// the plan first (every refusal; none needs the device), then the device: from its creation the env is owned by a handle that frees it, so no exit leaks
extern "C" int32_t uhc_env_create(UhcBatch* b, const UhcEnvDesc* d, UhcEnv** out) {
    if (!b || !d || !out) return uhc_internal_set_error("uhc_env_create: null argument");
    EnvArgs plan;
    const std::string refused = plan_env(uhc_internal_batch_info(b), *d, &plan);
    if (!refused.empty()) return uhc_internal_set_error(refused.c_str());

    std::unique_ptr<UhcEnv, void (*)(UhcEnv*)> owner(new UhcEnv(), uhc_env_free);
    UhcEnv* e = owner.get();
    e->b = b;
    e->E = plan;
    EnvArgs& E = e->E;
    const size_t N = E.n_env, nb = E.nbh - 1;
    double *w, *rjw;
    if (dalloc(e, nb, &w) || dalloc(e, nb, &rjw)) return 1;
    const std::vector<double> ones(nb, 1.0);
    HIP_OK(hipMemcpy(w, d->jpos_diffw, nb * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(rjw, d->reward_jpos_diffw ? d->reward_jpos_diffw : ones.data(), nb * sizeof(double), hipMemcpyHostToDevice));
    E.jpos_diffw = w, E.rjw = rjw;
    if (dalloc(e, N, &E.clip_id) || dalloc(e, N, &E.e_start) || dalloc(e, N, &E.e_len) || dalloc(e, N, &E.cur_t) || dalloc(e, N, &E.start_ind) ||
        dalloc(e, N * E.nu, &E.target_base) || dalloc(e, N * E.nq, &E.qpos_prev) || dalloc(e, N * E.obs_dim, &E.obs) || dalloc(e, N, &E.reward) ||
        dalloc(e, N * 6, &E.reward_parts) || dalloc(e, N, &E.height_lb) || dalloc(e, N, &E.percent) || dalloc(e, N, &E.body_diff) || dalloc(e, N, &E.done) || dalloc(e, N, &E.fail) ||
        dalloc(e, N, &E.end) || dalloc(e, N * E.nq, &e->stage_qpos) || dalloc(e, N * E.nv, &e->stage_qvel) || dalloc(e, N, &e->select) ||
        dalloc(e, N, &E.next_clip) || dalloc(e, N, &E.next_start) || dalloc(e, N, &E.next_len) || dalloc(e, N, &E.has_next) || dalloc(e, N, &E.consumed) ||
        dalloc(e, N * E.nu, &E.next_noise) || dalloc(e, 2 * N, &E.episode) || dalloc(e, 5 * N, &E.snapshot)) return 1;
    void* p; int64_t cnt;
    uhc_batch_field(b, UHC_F_QPOS, &p, &cnt); E.qpos = (const double*)p;
    uhc_batch_field(b, UHC_F_QVEL, &p, &cnt); E.qvel = (const double*)p;
    uhc_batch_field(b, UHC_F_XPOS, &p, &cnt); E.xpos = (const double*)p;
    uhc_batch_field(b, UHC_F_XQUAT, &p, &cnt); E.xquat = (const double*)p;
    uhc_batch_field(b, UHC_F_XIPOS, &p, &cnt); E.xipos = (const double*)p;
    uhc_batch_field(b, UHC_F_FAIL, &p, &cnt); E.sim_fail = (const int*)p;
    *out = owner.release();
    return 0;
}
extern "C" void uhc_env_free(UhcEnv* e) {
    if (!e) return;
    (void)hipDeviceSynchronize();
    for (void* p : e->allocs) (void)hipFree(p);
    delete e;
}
extern "C" int32_t uhc_env_obs_dim(const UhcEnv* e) { return e ? e->E.obs_dim : -1; }
extern "C" int32_t uhc_env_field(UhcEnv* e, int32_t f, void** p, int64_t* n) {
    if (!e) return uhc_internal_set_error("uhc_env_field: null env");
    const EnvArgs& E = e->E;
    const int64_t N = E.n_env;
    void* ptr = nullptr; int64_t cnt = 0;
    switch (f) {
        case UHC_E_OBS: ptr = E.obs; cnt = N * E.obs_dim; break;
        case UHC_E_REWARD: ptr = E.reward; cnt = N; break;
        case UHC_E_REWARD_PARTS: ptr = E.reward_parts; cnt = N * 6; break;
        case UHC_E_DONE: ptr = E.done; cnt = N; break;
        case UHC_E_FAIL: ptr = E.fail; cnt = N; break;
        case UHC_E_END: ptr = E.end; cnt = N; break;
        case UHC_E_PERCENT: ptr = E.percent; cnt = N; break;
        case UHC_E_CUR_T: ptr = E.cur_t; cnt = N; break;
        case UHC_E_BODY_DIFF: ptr = E.body_diff; cnt = N; break;
        case UHC_E_TARGET_BASE: ptr = E.target_base; cnt = N * E.nu; break;
        case UHC_E_CONSUMED: ptr = E.consumed; cnt = N; break;
        case UHC_E_EPISODE: ptr = E.episode; cnt = 2 * N; break;
        case UHC_E_SNAPSHOT: ptr = E.snapshot; cnt = 5 * N; break;
        case UHC_E_MODEL:
            if (!E.env_model) return uhc_internal_set_error("uhc_env_field: UHC_E_MODEL: a batch with one model keeps no per-env model");
            ptr = E.env_model; cnt = N; break;
        default: return uhc_internal_set_error("uhc_env_field: unknown field");
    }
    if (p) *p = ptr;
    if (n) *n = cnt;
    return 0;
}
extern "C" int32_t uhc_env_set_bank(UhcEnv* e, const double* d_frames, int64_t n_frames, const int32_t* d_clip_start,
                                    const double* d_clip_beta, int32_t n_clips) {
    if (!e || !d_frames || !d_clip_start || !d_clip_beta || n_frames < 1 || n_clips < 1) return uhc_internal_set_error("uhc_env_set_bank: bad argument");
    e->live.on = false;  // (a caller's bank ends live mode, like uhc_env_live_end)
    e->E.bank = d_frames; e->E.clip_start = d_clip_start; e->E.clip_beta = d_clip_beta;
    e->n_clips = n_clips; e->n_frames = n_frames;
    e->E.obj_pose = nullptr;  // rows of another bank
    return 0;
}
extern "C" int32_t uhc_env_set_obj_pose(UhcEnv* e, const double* d_obj_pose, int64_t n_frames) {
    if (!e) return uhc_internal_set_error("uhc_env_set_obj_pose: null env");
    NOT_WHILE_LIVE(e, "uhc_env_set_obj_pose");
    if (e->E.n_obj == 0) return d_obj_pose ? uhc_internal_set_error("uhc_env_set_obj_pose: the env was created with num_obj = 0") : 0;
    if (!d_obj_pose || !e->E.bank || n_frames != e->n_frames) return uhc_internal_set_error("uhc_env_set_obj_pose: one row of 7 num_obj numbers per frame of the clip bank (set the bank first)");
    e->E.obj_pose = d_obj_pose;
    return 0;
}
extern "C" int32_t uhc_env_set_clip_models(UhcEnv* e, const int32_t* d_clip_model) {
    if (!e) return uhc_internal_set_error("uhc_env_set_clip_models: null env");
    NOT_WHILE_LIVE(e, "uhc_env_set_clip_models");
    int n_models = 1;
    int* em = uhc_internal_env_model(e->b, &n_models);
    if (d_clip_model && (!em || n_models < 2)) return uhc_internal_set_error("uhc_env_set_clip_models: the batch was created with a single model");
    e->E.clip_model = d_clip_model;
    e->E.env_model = em;
    return 0;
}
extern "C" int32_t uhc_env_assign(UhcEnv* e, const int32_t* ids, int32_t n, const int32_t* clip_ids, const int32_t* fr_start, const int32_t* fr_len) {
    if (!e || !ids || !clip_ids || !fr_start || !fr_len || n < 1) return uhc_internal_set_error("uhc_env_assign: bad argument");
    NOT_WHILE_LIVE(e, "uhc_env_assign");
    if (!e->E.bank) return uhc_internal_set_error("uhc_env_assign: no clip bank set");
    HIP_OK(uhc_launch_env_assign(&e->E, ids, n, clip_ids, fr_start, fr_len, stream_of(e)));
    return 0;
}
extern "C" int32_t uhc_env_reset(UhcEnv* e, const int32_t* ids, int32_t n, const double* d_noise) {
    if (!e || !ids || n < 1 || n > e->E.n_env) return uhc_internal_set_error("uhc_env_reset: bad argument");
    if (!e->E.bank) return uhc_internal_set_error("uhc_env_reset: no clip bank set");
    if (e->E.n_obj > 0 && !e->E.obj_pose) return uhc_internal_set_error("uhc_env_reset: the model has objects but no obj_pose rows are set (uhc_env_set_obj_pose)");
    hipStream_t s = stream_of(e);
    HIP_OK(uhc_launch_env_reset_stage(&e->E, ids, n, d_noise, e->stage_qpos, e->stage_qvel, s));
    if (uhc_batch_set_state(e->b, ids, n, e->stage_qpos, e->stage_qvel)) return 1;  // set_state + forward on those envs
    HIP_OK(uhc_launch_env_post(1, &e->E, nullptr, uhc_internal_reset_mask(e->b), s));  // observation of the reset envs (mask = envs just reset)
    return 0;
}
extern "C" int32_t uhc_env_set_next(UhcEnv* e, const int32_t* ids, int32_t n, const int32_t* clip_ids, const int32_t* fr_start, const int32_t* fr_len,
                                    const double* d_noise) {
    if (!e || !ids || !clip_ids || !fr_start || !fr_len || n < 1 || n > e->E.n_env) return uhc_internal_set_error("uhc_env_set_next: bad argument");
    NOT_WHILE_LIVE(e, "uhc_env_set_next");
    if (!e->E.bank) return uhc_internal_set_error("uhc_env_set_next: no clip bank set");
    HIP_OK(uhc_launch_env_set_next(&e->E, ids, n, clip_ids, fr_start, fr_len, d_noise, stream_of(e)));
    return 0;
}
extern "C" int32_t uhc_env_set_end_reward(UhcEnv* e, double end_reward) {
    if (!e) return uhc_internal_set_error("uhc_env_set_end_reward: null env");
    e->E.end_reward = end_reward;
    return 0;
}
extern "C" int32_t uhc_env_auto_reset(UhcEnv* e) {
    if (!e) return uhc_internal_set_error("uhc_env_auto_reset: null env");
    NOT_WHILE_LIVE(e, "uhc_env_auto_reset");
    if (!e->E.bank) return uhc_internal_set_error("uhc_env_auto_reset: no clip bank set");
    if (e->E.n_obj > 0 && !e->E.obj_pose) return uhc_internal_set_error("uhc_env_auto_reset: the model has objects but no obj_pose rows are set (uhc_env_set_obj_pose)");
    hipStream_t s = stream_of(e);
    HIP_OK(uhc_launch_env_auto_stage(&e->E, e->stage_qpos, e->stage_qvel, e->select, s));
    if (uhc_internal_set_state_masked(e->b, e->select, e->stage_qpos, e->stage_qvel)) return 1;
    HIP_OK(uhc_launch_env_post(1, &e->E, nullptr, e->select, s));
    return 0;
}
extern "C" int32_t uhc_env_step(UhcEnv* e, const double* d_action, const int32_t* d_active) {
    if (!e || !d_action) return uhc_internal_set_error("uhc_env_step: bad argument");
    if (!e->E.bank) return uhc_internal_set_error("uhc_env_step: no clip bank set");
    hipStream_t s = stream_of(e);
    HIP_OK(uhc_launch_env_pre(&e->E, d_active, s));
    if (uhc_batch_simulate(e->b, d_action, e->E.target_base, d_active)) return 1;
    HIP_OK(uhc_launch_env_post(0, &e->E, d_action, d_active, s));
    return 0;
}

// ------------------------------------------------------------------ live targets (include/uhc_amd.h, "live targets"); the kernel is uhc_live.hip's
static void* take_alloc(UhcEnv* e, void* p) {  // p leaves the env's allocation list (to be freed by the caller)
    for (size_t i = 0; i < e->allocs.size(); i++)
        if (e->allocs[i] == p) { e->allocs.erase(e->allocs.begin() + i); break; }
    return p;
}
extern "C" int32_t uhc_env_live_begin(UhcEnv* e, int32_t cap, int32_t n_body, const int32_t* h_parent, const int32_t* h_ee_body, const double* d_body_pos,
                                      const double* d_body_ipos, int32_t n_models, double dt, const double* d_beta) {
    // the checks that do not read the env come first; e == NULL is the last one before any HIP call
    if (cap < 2) return uhc_internal_set_error("uhc_env_live_begin: cap must be at least 2 (a stream needs a pair of frames for its velocities)");
    if (n_body != XF_NBODY) return uhc_internal_set_error("uhc_env_live_begin: n_body must be 24 (UHC_FRAME_STRIDE is a 24-body layout)");
    if (!h_parent) return uhc_internal_set_error("uhc_env_live_begin: h_parent is NULL");
    if (!h_ee_body) return uhc_internal_set_error("uhc_env_live_begin: h_ee_body is NULL");
    if (!d_body_pos) return uhc_internal_set_error("uhc_env_live_begin: d_body_pos is NULL");
    if (!d_body_ipos) return uhc_internal_set_error("uhc_env_live_begin: d_body_ipos is NULL");
    if (n_models <= 0) return uhc_internal_set_error("uhc_env_live_begin: n_models <= 0");
    if (!(dt > 0.0)) return uhc_internal_set_error("uhc_env_live_begin: dt <= 0");
    XfTree tree;
    const std::string bad = xf_tree_fill("uhc_env_live_begin", h_parent, h_ee_body, &tree);
    if (!bad.empty()) return uhc_internal_set_error(bad.c_str());
    if (!e) return uhc_internal_set_error("uhc_env_live_begin: the env e is NULL");
    int batch_models = 1;
    int* em = uhc_internal_env_model(e->b, &batch_models);
    if (n_models != batch_models)
        return uhc_internal_set_error(("uhc_env_live_begin: n_models = " + std::to_string(n_models) + ", the batch was created with " + std::to_string(batch_models)).c_str());
    if (e->E.n_obj > 0) return uhc_internal_set_error("uhc_env_live_begin: the env was created with num_obj > 0 (object poses per live frame are not supported)");
    const size_t N = e->E.n_env;
    if ((long long)N * cap > 0x7fffffffLL) return uhc_internal_set_error("uhc_env_live_begin: n_env x cap is beyond 2^31 - 1 frames");
    HIP_OK(hipStreamSynchronize(stream_of(e)));  // (a step in flight may still read the bank the tables below are about to clear)
    if (cap > e->live.alloc_cap) {
        if (e->live.on) (void)uhc_env_live_end(e);  // (the bank about to be freed may be the installed one: no bank until this call succeeds)
        if (e->live.bank) (void)hipFree(take_alloc(e, e->live.bank));
        e->live.bank = nullptr, e->live.alloc_cap = 0;
        void* q = nullptr;
        if (hipMalloc(&q, N * cap * UHC_FRAME_STRIDE * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            return uhc_internal_set_error(("uhc_env_live_begin: cap = " + std::to_string(cap) + ": no memory for n_env x cap x 4672 bytes").c_str());
        }
        e->allocs.push_back(q);
        e->live.bank = (double*)q, e->live.alloc_cap = cap;
    }
    if (!e->live.len && (dalloc(e, N * XF_NQ, &e->live.prev_qpos) || dalloc(e, N, &e->live.len) || dalloc(e, N, &e->live.dropped) ||
                         dalloc(e, N, &e->live.clip_start) || dalloc(e, N * 17, &e->live.beta) || dalloc(e, N, &e->live.base) || dalloc(e, N, &e->live.moved) ||
                         dalloc(e, (size_t)n_models * XF_NBODY * 3, &e->live.body_pos) || dalloc(e, (size_t)n_models * XF_NBODY * 3, &e->live.body_ipos)))
        return 1;
    hipStream_t s = stream_of(e);
    HIP_OK(hipMemsetAsync(e->live.len, 0, N * sizeof(int), s));  // every stream is cleared: an append without a restart is dropped
    HIP_OK(hipMemsetAsync(e->live.dropped, 0, N * sizeof(int), s));
    HIP_OK(hipMemsetAsync(e->live.base, 0, N * sizeof(int), s));
    HIP_OK(hipMemsetAsync(e->live.moved, 0, N * sizeof(int), s));
    HIP_OK(hipMemsetAsync(e->live.prev_qpos, 0, N * XF_NQ * sizeof(double), s));
    // every slot is zeroed and every env points at a window of ONE frame inside its own stream: a reset or a step before the first push reads zeros,
    // never a frame outside the bank (the env kernels clamp to e_len - 1, and e_start of an earlier bank means nothing here)
    HIP_OK(hipMemsetAsync(e->live.bank, 0, N * cap * UHC_FRAME_STRIDE * sizeof(double), s));
    std::vector<int> cs(N), ones(N, 1), iota(N);
    for (size_t i = 0; i < N; i++) cs[i] = (int)(i * cap), iota[i] = (int)i;
    HIP_OK(hipMemcpy(e->live.clip_start, cs.data(), N * sizeof(int), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(e->E.e_start, cs.data(), N * sizeof(int), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(e->E.e_len, ones.data(), N * sizeof(int), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(e->E.clip_id, iota.data(), N * sizeof(int), hipMemcpyHostToDevice));
    if (d_beta) HIP_OK(hipMemcpy(e->live.beta, d_beta, N * 17 * sizeof(double), hipMemcpyDeviceToDevice));
    else HIP_OK(hipMemset(e->live.beta, 0, N * 17 * sizeof(double)));
    HIP_OK(hipMemcpy(e->live.body_pos, d_body_pos, (size_t)n_models * XF_NBODY * 3 * sizeof(double), hipMemcpyDeviceToDevice));
    HIP_OK(hipMemcpy(e->live.body_ipos, d_body_ipos, (size_t)n_models * XF_NBODY * 3 * sizeof(double), hipMemcpyDeviceToDevice));
    HIP_OK(hipStreamSynchronize(s));
    e->live.on = true, e->live.slide = false, e->live.cap = cap, e->live.models = n_models, e->live.dt = dt, e->live.tree = tree;
    e->E.bank = e->live.bank, e->E.clip_start = e->live.clip_start, e->E.clip_beta = e->live.beta;
    e->E.obj_pose = nullptr, e->E.clip_model = nullptr, e->E.env_model = em;
    e->n_clips = (int)N, e->n_frames = (int64_t)N * cap;
    return 0;
}
extern "C" int32_t uhc_env_live_push(UhcEnv* e, const int32_t* d_env_ids, int32_t n, const double* d_qpos, const double* d_root_quat_record,
                                     const int32_t* d_restart, const int32_t* d_model) {
    if (!d_env_ids) return uhc_internal_set_error("uhc_env_live_push: d_env_ids is NULL");
    if (!d_qpos) return uhc_internal_set_error("uhc_env_live_push: d_qpos is NULL");
    if (n < 0) return uhc_internal_set_error("uhc_env_live_push: n < 0");
    if (n == 0) return 0;  // (nothing to push: no launch, and nothing of the env is read)
    if (!e) return uhc_internal_set_error("uhc_env_live_push: the env e is NULL");
    if (!e->live.on) return uhc_internal_set_error("uhc_env_live_push: the env is not in live mode (uhc_env_live_begin)");
    HIP_OK(uhc_launch_live_push(&e->E, &e->live, d_env_ids, n, d_qpos, d_root_quat_record, d_restart, d_model, stream_of(e)));
    return 0;
}
extern "C" int32_t uhc_env_live_slide(UhcEnv* e, int32_t on) {
    if (!e) return uhc_internal_set_error("uhc_env_live_slide: the env e is NULL");
    if (!e->live.on) return uhc_internal_set_error("uhc_env_live_slide: the env is not in live mode (uhc_env_live_begin)");
    if (on && e->E.obs_v == 0 && (e->E.obs_flags & 4))
        return uhc_internal_set_error("uhc_env_live_slide: the env's observation carries the phase word (obs_v 0 with obs_flags & 4): cur_t / len would jump at a slide");
    e->live.slide = on != 0;
    return 0;
}
extern "C" int32_t uhc_env_live_window(UhcEnv* e, int32_t** d_base, int32_t** d_moved) {
    if (!e) return uhc_internal_set_error("uhc_env_live_window: the env e is NULL");
    if (!e->live.on) return uhc_internal_set_error("uhc_env_live_window: the env is not in live mode (uhc_env_live_begin)");
    if (d_base) *d_base = e->live.base;
    if (d_moved) *d_moved = e->live.moved;
    return 0;
}
extern "C" int32_t uhc_env_live_view(UhcEnv* e, double** d_frames, int32_t** d_len, int32_t** d_dropped, int32_t* cap) {
    if (!e) return uhc_internal_set_error("uhc_env_live_view: the env e is NULL");
    if (!e->live.on) return uhc_internal_set_error("uhc_env_live_view: the env is not in live mode (uhc_env_live_begin)");
    if (d_frames) *d_frames = e->live.bank;
    if (d_len) *d_len = e->live.len;
    if (d_dropped) *d_dropped = e->live.dropped;
    if (cap) *cap = e->live.cap;
    return 0;
}
extern "C" int32_t uhc_env_live_end(UhcEnv* e) {
    if (!e) return uhc_internal_set_error("uhc_env_live_end: the env e is NULL");
    if (!e->live.on) return uhc_internal_set_error("uhc_env_live_end: the env is not in live mode (uhc_env_live_begin)");
    e->live.on = false;
    e->E.bank = nullptr, e->E.clip_start = nullptr, e->E.clip_beta = nullptr, e->E.clip_model = nullptr;
    e->n_clips = 0, e->n_frames = 0;
    return 0;
}
