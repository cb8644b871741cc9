// env_plan_probe.cpp -- plan_env (uhc_amd/csrc/uhc_env_plan.h), the pure part of uhc_env_create, behind a C entry for tests/test_env_plan_cpu.py.
// Host compiler only: no HIP header, no device.
#include <cstring>

#include "uhc_env_plan.h"

#define PROBE extern "C" __attribute__((visibility("default")))

// dims: n_env nq nv nu nbody action_dim vf_dim n_trailing_free.  Returns 0 and the plan's scalars, or 1 and the refusal's text in err.
// ints: n_obj nqh nvh nbh ball has_shape obs_v reward_v obs_flags term_body obs_dim fut_frames fut_skip env_episode_len expert_trail_steps | ee_body[5] |
//       n_env nq nv nu nbody action_dim vf_dim (27); doubles: dt body_diff_thresh | rw[16] | base_rot_inv[4] (22); set_pointers: how many of seven of E's pointers are not null
PROBE int uhc_env_plan_probe(const int* dims, double dt, const double* base_rot_inv, const UhcEnvDesc* d, int* ints, double* doubles, int* set_pointers, char* err,
                             int err_cap) {
    UhcBatchInfo B = {};
    B.n_env = dims[0], B.nq = dims[1], B.nv = dims[2], B.nu = dims[3], B.nbody = dims[4], B.action_dim = dims[5], B.vf_dim = dims[6], B.n_trailing_free = dims[7];
    B.dt = dt;
    for (int k = 0; k < 4; k++) B.base_rot_inv[k] = base_rot_inv[k];
    EnvArgs E;
    memset(&E, 0xff, sizeof E);  // (what plan_env does not set would show)
    const std::string bad = plan_env(B, *d, &E);
    if (!bad.empty()) {
        strncpy(err, bad.c_str(), err_cap - 1);
        err[err_cap - 1] = 0;
        return 1;
    }
    const int v[27] = {E.n_obj, E.nqh, E.nvh, E.nbh, E.ball, E.has_shape, E.obs_v, E.reward_v, E.obs_flags, E.term_body, E.obs_dim, E.fut_frames, E.fut_skip,
                       E.env_episode_len, E.expert_trail_steps, E.ee_body[0], E.ee_body[1], E.ee_body[2], E.ee_body[3], E.ee_body[4],
                       E.n_env, E.nq, E.nv, E.nu, E.nbody, E.action_dim, E.vf_dim};
    memcpy(ints, v, sizeof v);
    doubles[0] = E.dt, doubles[1] = E.body_diff_thresh;
    for (int k = 0; k < 16; k++) doubles[2 + k] = E.rw[k];
    for (int k = 0; k < 4; k++) doubles[18 + k] = E.base_rot_inv[k];
    *set_pointers = (E.bank != nullptr) + (E.obs != nullptr) + (E.qpos != nullptr) + (E.jpos_diffw != nullptr) + (E.env_model != nullptr) + (E.obj_pose != nullptr) +
                    (E.snapshot != nullptr);
    return 0;
}
