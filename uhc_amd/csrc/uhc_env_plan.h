// uhc_env_plan.h -- what an env IS, decided without the device: the pure part of uhc_env_create (uhc_env_capi.cpp), shared with a host build
// (tests/env_plan_probe.cpp).  From the batch's dims and the caller's descriptor: the humanoid's extents in front of the objects, hinge or ball, the
// observation's width, and every refusal that needs no device.  Nothing of the HIP runtime.
#pragma once
#include <cstring>
#include <string>

#include "../../include/uhc_amd.h"
#include "uhc_device_env.h"

// what the env layer reads of a batch (uhc_internal_batch_info, uhc_capi.cpp): fixed at uhc_batch_create
struct UhcBatchInfo {
    int n_env, nq, nv, nu, nbody, action_dim, vf_dim;
    double dt;               // of a control step: timestep x substeps
    double base_rot_inv[4];
    int n_trailing_free;     // free bodies at the end of the model: the most objects an env may claim
};
extern "C" UhcBatchInfo uhc_internal_batch_info(UhcBatch* b);  // the one declaration: uhc_capi.cpp defines it, uhc_env_capi.cpp calls it (see uhc_internal.h)

// The width of one observation frame.  nb: the humanoid's non-root bodies; shape: beta(16) + gender when the env appends them.  One expression per
// version, beside the lines of the reference's humanoid_im.py it restates.
inline int env_obs_frame_dim(int obs_v, bool ball, int flags, int nqh, int nvh, int nu, int nb, int shape) {
    if (ball) return 7 + 4 * nb + (nu + 6) + 3 + 6 * nb + 8 * nb + shape;  // get_full_obs_v2_quat (:668-756); the ball env has no other
    switch (obs_v) {
        // get_full_obs (:290-317): [heading] qpos[2:] velocities (the root's 6 under obs_vel "root", all under "full") expert joint angles [phase]; never the shape
        case 0: return (flags & 1) + (nqh - 2) + ((flags & 8) ? 6 : nvh) + nu + ((flags >> 2) & 1);
        case 1: return 304 + 20 * nb + shape;                       // get_full_obs_v1 (:323-417)
        case 2: return 304 + 14 * nb + shape;                       // get_full_obs_v2 (:419-503)
        case 3: return 304 + 14 * nb + shape;                       // get_full_obs_v3 (:758-767): fut_frames frames of v2
        case 4: return 28 + 26 * (nb - 1) + shape;                  // get_full_obs_v4 (:769-861): global block | shape | one row of 26 per non-root body
        case 5: return 300 + 14 * nb + shape;                       // get_full_obs_v5 (:505-594)
        default: return 8 + nvh + 2 * nb + 11 * (nb - 1) + shape;   // get_full_obs_v6 (:596-666)
    }
}

// B, d -> the scalar part of *E (every pointer null); "" or why the descriptor is refused -- in the order a caller with two faults has always been told
inline std::string plan_env(const UhcBatchInfo& B, const UhcEnvDesc& d, EnvArgs* out) {
    if (d.obs_v < 0 || d.obs_v > 6) return "uhc_env_create: obs_v must be 0 .. 6";
    if (d.obs_v == 3 && (d.fut_frames < 1 || d.fut_frames > 64 || d.fut_skip < 0)) return "uhc_env_create: obs_v 3 needs 1 <= fut_frames <= 64, skip >= 0";
    if (d.term_body != 0 && d.term_body != 1) return "uhc_env_create: term_body must be 0 (cfg.env_term_body 'body') or 1 ('root')";
    if (d.reward_v < 0 || d.reward_v > 5) return "uhc_env_create: reward_v must be 0 .. 5 (implicit, explicit, implicit_v1_mul, explicit_mul, implicit_v2, implicit_v3)";
    EnvArgs& E = *out;
    memset(&E, 0, sizeof E);
    E.n_env = B.n_env; E.nq = B.nq; E.nv = B.nv; E.nu = B.nu; E.nbody = B.nbody; E.action_dim = B.action_dim; E.vf_dim = B.vf_dim; E.dt = B.dt;
    for (int k = 0; k < 4; k++) E.base_rot_inv[k] = B.base_rot_inv[k];
    // free objects (expert["obj_pose"], humanoid_im.py:1284-1287): the LAST num_obj bodies of the model, one free joint each; what is in front of
    // them is the humanoid -- the reference's qpos_lim / qvel_lim / body_lim (humanoid_im.py:113-115), which its observations, rewards and
    // termination stop at
    E.n_obj = d.num_obj;
    if (E.n_obj < 0 || E.n_obj > B.n_trailing_free) return "uhc_env_create: num_obj exceeds the free bodies at the end of the model";
    E.nqh = E.nq - 7 * E.n_obj; E.nvh = E.nv - 6 * E.n_obj; E.nbh = E.nbody - E.n_obj;
    const int nb = E.nbh - 1;
    // ball-joint humanoid (robot.ball): free root + one ball joint per further body
    E.ball = E.nqh == 7 + 4 * (nb - 1) && E.nvh == 6 + 3 * (nb - 1) && nb > 1 && E.nqh != E.nvh + 1;
    if ((E.nqh != E.nvh + 1 && !E.ball) || E.nq > 192 || nb < 1 || nb > 64) return "uhc_env_create: hinge humanoid (free root + scalar joints) or ball-joint humanoid (free root + one ball joint per body), followed by num_obj free bodies, nq <= 192, expected";
    if (E.ball && (d.obs_v != 2 || d.reward_v != 0)) return "uhc_env_create: the ball-joint env has observation v2 (get_full_obs_v2_quat) and reward 0 (world_rfc_implicit_quat)";
    E.obs_v = d.obs_v;
    E.reward_v = d.reward_v;
    E.obs_flags = d.obs_flags;
    E.term_body = d.term_body;
    E.has_shape = d.obs_v == 0 ? 0 : d.has_shape;
    E.fut_frames = d.obs_v == 3 ? d.fut_frames : 1;
    E.fut_skip = d.obs_v == 3 ? d.fut_skip : 0;
    E.obs_dim = E.fut_frames * env_obs_frame_dim(d.obs_v, E.ball != 0, d.obs_flags, E.nqh, E.nvh, E.nu, nb, d.has_shape ? 17 : 0);
    E.env_episode_len = d.env_episode_len;
    E.expert_trail_steps = d.env_expert_trail_steps;
    for (int k = 0; k < 5; k++) E.ee_body[k] = d.ee_body[k];
    E.body_diff_thresh = d.body_diff_thresh;
    for (int k = 0; k < 16; k++) E.rw[k] = d.reward_weights[k];
    return std::string();
}
