"""Tracking a live source: a frozen imitation policy follows target poses that arrive one per control step (a kinematic policy as in the
reference's uhc/envs/humanoid_kin_v1.py, a pose estimator, a motion generator, teleoperation).  The targets go into the envs' streams with
`VecHumanoidEnv.live_push` (uhc_env_live_push: one launch, no host FK, no upload of frame records, no new clip bank); the policy and the filter are the
caller's -- run by the framework (policy="torch"), or copied once into the library's frozen policy (policy="device": uhc_amd.policy_ops.DevicePolicy, one
uhc_policy_act per step from the env's raw observation to the action tensor).  Nothing here reads the device back: `step` returns views."""
from __future__ import annotations

import torch

from . import sim as S


class StreamTracker:
    """env: a `VecHumanoidEnv` in live mode (`env.live_begin(cap)`); policy_net: a policy with `select_action(state, mean_action)`; running_state: the
    policy's observation filter (ZFilter) or None -- applied with update=False, the statistics are those the policy was trained with.
    A session of any length: `env.live_begin(cap, slide=True)` with cap a few times the head (at least head + 1) -- the window slides under the envs as
    `step` pushes, nothing else changes here; without slide, cap bounds the session and later rows are dropped.
    policy: "torch" -- the framework runs filter and policy_net --, or "device" -- the weights and the filter's statistics AS THEY ARE NOW are copied into a
    `DevicePolicy` (policy_net may be one already: running_state is then ignored, the filter is inside it); every step reads `env.obs` where it lies, with
    the filter fused into the first layer, and writes one fixed action tensor that `env.step` takes."""

    def __init__(self, env, policy_net, running_state=None, dtype=torch.float64, policy="torch"):
        if policy not in ("torch", "device"):
            raise ValueError(f"StreamTracker: policy is 'torch' or 'device', got {policy!r}")
        self.env, self.policy_net, self.running_state, self.dtype = env, policy_net, running_state, dtype
        self.device_policy = None
        if policy == "device":
            from .policy_ops import DevicePolicy
            self.device_policy = policy_net if isinstance(policy_net, DevicePolicy) else DevicePolicy.from_modules(policy_net, running_state, max_rows=env.n_env,
                                                                                                                    device=env.device)
            self._action = torch.zeros((env.n_env, self.device_policy.act_dim), dtype=torch.float64, device=env.device)
        self._ids = torch.arange(env.n_env, dtype=torch.int32, device=env.device)
        self._ones = torch.ones(env.n_env, dtype=torch.int32, device=env.device)

    def _state(self):
        obs = self.env.obs.to(self.dtype)
        return self.running_state(obs, update=False) if self.running_state is not None else obs

    def begin(self, head, root_quat_record=None):
        """head (n_env, k >= 2, 76): the first k target rows of every env's stream (device or host).  Frame 0 restarts the streams, the others are
        appended, the envs are reset onto frame 0; returns the observation view.  root_quat_record (n_env, k, 4): the ball-joint humanoid's.
        (On a sliding env k <= cap - 1, so that the first push after the reset finds room.)"""
        head = torch.as_tensor(head).to(self.env.device, torch.float64)
        if head.ndim != 3 or head.shape[0] != self.env.n_env or head.shape[1] < 2 or head.shape[2] != 76:
            raise ValueError(f"StreamTracker.begin: head must be ({self.env.n_env}, k >= 2, 76), got {tuple(head.shape)}")
        for t in range(head.shape[1]):
            self.env.live_push(self._ids, head[:, t].contiguous(), restart=self._ones if t == 0 else None,
                               root_quat_record=None if root_quat_record is None else torch.as_tensor(root_quat_record)[:, t])
        self.env.reset(self._ids)
        return self.env.obs

    def step(self, next_qpos=None, restart=None, root_quat_record=None, smpl=False):
        """One control step of every env: mean action of the policy on the filtered observation; `next_qpos` (n_env, 76), when given, is appended to the
        streams BEFORE the step (restart (n_env,): non-zero rows start a new stream instead -- the caller resets those envs).  Returns (qpos view
        (n_env, nq), done view (n_env,)); with smpl=True (qpos, done, pose_aa (n_env, 72), trans (n_env, 3)): the state after the step in the form the
        targets came in (`VecHumanoidEnv.smpl_pose`: one more launch, no readback; the env's own tensors, written again by the next such step)."""
        if self.device_policy is not None:
            action = self.device_policy.mean(self.env.obs, out=self._action)
        else:
            with torch.no_grad():
                action = self.policy_net.select_action(self._state(), True).to(torch.float64).contiguous()
        if next_qpos is not None:
            self.env.live_push(self._ids, next_qpos, restart=restart, root_quat_record=root_quat_record)
        self.env.step(action)
        if smpl:
            return (self.env.sim.field(S.F_QPOS), self.env.done) + self.env.smpl_pose(("pose_aa", "trans"))
        return self.env.sim.field(S.F_QPOS), self.env.done
