"""The env kernels (uhc_env.hip) at their branch edges, against the float64 oracle evaluated ON THE DEVICE'S OWN STATE: after a reset or a
step the test reads qpos, qvel, xpos, xquat and xipos back and hands them, with the clip-bank records it wrote itself, to oracle/env_oracle.py.
No OracleSim steps beside the device, so what is compared is the env arithmetic alone and the tolerance is a rounding-noise bar.

Cases (tests/env_edge_cases.py; tests/test_env_edge_cases_cpu.py proves each reaches its branch): root yaw in all quadrants as q and -q, heading
differences beyond +-pi for the acos and the atan2 heading, pitch / roll to sqrt(w^2 + z^2) = 1.7e-3, root world quaternion with w == 0.0
(`unset`), off-unit root quaternions, joints on and beyond their limits with velocities of +-50, windows of 1 / 2 / 3 / 7 / 12 frames, five clips
behind large offsets and a permuted strict subset of env ids; expert quaternions equal / negated / 90 / 179.9 / 359.9 degrees away / scaled,
termination distance 1e-9 either side of two thresholds, nine distinct residual entries per body, trail steps, episode length, episode accounting.

Tolerance: per entry 16 x the spread of the oracle over its inputs and 8 copies moved by one float64 step each, + 1e-14 max(1, |value|)
(env_edge_cases.measured_bar).  Largest bars, as derived on the CPU stand-in states: observations v1-v4 2.2e-12, v5 7.3e-13, v6 9.9e-13, ball
1.1e-12 (all at the 1.7e-3 heading norm / +-50 velocities; median case 6e-14); v0 below those; reward and parts 6.0e-13 (ball 2.5e-12), except
next to acos(-1) -- negated and 359.9-degree targets -- where one rounding of the argument moves acos by 1.5e-8 and the bar is 2.1e-8.

On the device states the bars come out at 1e-14 .. 4e-14 for the observations and 1e-14 .. 8e-13 for the rewards, and the device stays below 0.15 of them
everywhere.  (The v0 heading at a yaw of +-1e-3 has a bar of 1e-14 -- moving w and z by one step does not move w / sqrt(w^2 + z^2) = 1 - 1.25e-7 at all --
while one step of that quotient is 4.4e-13 of heading: it holds because heading() forms the norm in the order np.linalg.norm does.)  The reset copies an off-unit root quaternion into qpos as it is (norm 1.001 stays 1.001); only
the world quaternions are normalised.  `bd_eq0.5` is the one case ON a switch: a termination distance of exactly 0.5 in exact arithmetic (no bar involved).

Not reached: the |1 -+ dq0| < 1e-6 shortcut of the finite-difference angular velocity (needs a body that did not rotate during a step)."""
import os

import numpy as np
import pytest

from tests import env_edge_cases as C

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = -7.25e7
N_ENV_OBS = 48


@pytest.fixture(scope="module")
def humanoid(model):
    from uhc_amd.smpllib.torch_smpl_humanoid import Humanoid
    return Humanoid(model=model)


@pytest.fixture(scope="module")
def obs_table(humanoid):
    cases = C.obs_cases()
    wins = C.obs_windows(humanoid, cases)
    return cases, wins, C.assemble_bank(wins)


@pytest.fixture(scope="module")
def walk():
    return np.load(os.path.join(G, "g3_qpos_fk.npz"))["f_qpos"]


def _make(model, kind, n_env, rv=0, ctrl=None, explicit=False, **desc):
    """SimBatch + EnvBatch of one flavour; `kind` is the observation version or "ball" (ball-joint model, torque control, no residual force)."""
    import dataclasses
    from uhc_amd import sim as S
    from uhc_amd._capi import env_desc
    from uhc_amd.model.mjcf import ball_variant
    from uhc_amd.smpllib.smpl_mujoco import SMPLConverter
    ball = kind == "ball"
    if ball:
        ctrl = S.make_ctrl(model, action_type="torque", residual_force=False, meta_pd=False, tq_mul=4)
    elif explicit:
        ctrl = S.make_ctrl(model, residual_force_mode="explicit")
    sb = S.SimBatch(dataclasses.replace(ball_variant(model), solver=1) if ball else model, ctrl, n_env)
    eb = S.EnvBatch(sb, env_desc(model, obs_v=2 if ball else kind, has_shape=kind != 1, reward_v=rv, fut_frames=C.FUT_FRAMES, fut_skip=C.FUT_SKIP, obs_heading=True,
                                 root_deheading=True, obs_phase=True, jpos_diffw=SMPLConverter(model, model).get_new_diff_weight(), **desc))
    assert eb.obs_dim == C.OBS_DIM[kind]
    return sb, eb, ctrl


def _set_bank(eb, bank):
    import torch
    frames, clip_start, _ = bank
    eb.set_bank(torch.from_numpy(frames), torch.from_numpy(clip_start), torch.from_numpy(C.clip_beta_rows()))


def _assign_reset(eb, ids, where):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))  # noqa: E731
    eb.assign(t(ids), t(where[:, 0]), t(where[:, 1]), t(where[:, 2]))
    eb.reset(t(ids).cuda(), None)
    eb.sim.sync()


def _readback(sb):
    from uhc_amd import sim as S
    n = sb.n_env
    g = lambda f: sb.field(f).cpu().numpy().copy()  # noqa: E731
    return dict(qpos=g(S.F_QPOS), qvel=g(S.F_QVEL), xpos=g(S.F_XPOS).reshape(n, -1, 3), xquat=g(S.F_XQUAT).reshape(n, -1, 4), xipos=g(S.F_XIPOS).reshape(n, -1, 3))


def _state(rb, e):
    return {k: rb[k][e] for k in C.STATE_KEYS}


class _Worst:
    """Every entry of a block against its bar: the misses are collected and asserted together, the largest deviation / bar ratio is printed
    (run with -s) for the record."""

    def __init__(self, label):
        self.label, self.ratio, self.dev, self.bar, self.where, self.misses = label, 0.0, 0.0, 0.0, "", []

    def check(self, got, ref, bar, where):
        got, ref, bar = np.atleast_1d(got), np.atleast_1d(ref), np.atleast_1d(bar)
        assert got.shape == ref.shape, (where, got.shape, ref.shape)
        d = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
        i = int(np.argmax(d / bar))
        if d[i] / bar[i] > self.ratio:
            self.ratio, self.dev, self.bar, self.where = d[i] / bar[i], d[i], bar[i], f"{where}[{i}]"
        for j in np.nonzero(d > bar)[0][:4]:
            self.misses.append(f"{where}[{j}]: off by {d[j]:.3e}, bar {bar[j]:.3e} (device {got[j]!r}, oracle {ref[j]!r})")

    def report(self):
        print(f"\nEDGE {self.label}: largest deviation/bar {self.ratio:.3f} (deviation {self.dev:.2e}, bar {self.bar:.2e}) at {self.where}")
        assert not self.misses, f"{self.label}: {len(self.misses)} entries beyond their bar:\n" + "\n".join(self.misses[:12])


# ----------------------------------------------------------------------------------------------------------- 1. observations on the reset path
def _reset_observation(model, ctrl, obs_table, kind):
    from uhc_amd import sim as S
    cases, wins, bank = obs_table
    where = bank[2]
    ball = kind == "ball"
    sb, eb, _ = _make(model, kind, N_ENV_OBS, ctrl=ctrl)
    _set_bank(eb, bank)
    eb.field(S.E_OBS).fill_(SENTINEL)
    ids = C.env_ids_for(len(cases), N_ENV_OBS)
    _assign_reset(eb, ids, where)
    rb = _readback(sb)
    gobs = eb.field(S.E_OBS).cpu().numpy()
    others = np.setdiff1d(np.arange(N_ENV_OBS), ids)
    assert len(others) > 0 and (gobs[others] == SENTINEL).all()  # envs outside the id list are untouched
    assert eb.field(S.E_CUR_T).cpu().numpy()[ids].tolist() == [0] * len(ids)
    beta = C.clip_beta_rows()
    worst = _Worst(f"obs {kind}")
    for i, (c, w) in enumerate(zip(cases, wins)):
        env = int(ids[i])
        st = _state(rb, env)
        # the reset put the env on frame 0 of its own window (velocity: the window's second frame, its own if it has one frame)
        want = C.stand_in_state(w, ball=ball)
        assert np.array_equal(st["qpos"][:3], want["qpos"][:3]), c["name"]
        if ball:  # (the forward pass may renormalise the joint quaternions in place: one rounding)
            np.testing.assert_allclose(st["qpos"][7:], want["qpos"][7:], atol=1e-15)
        else:
            assert np.array_equal(st["qpos"][7:], want["qpos"][7:]), c["name"]
        np.testing.assert_allclose(st["qpos"][3:7] / np.linalg.norm(st["qpos"][3:7]), want["qpos"][3:7] / np.linalg.norm(want["qpos"][3:7]), atol=1e-15)
        assert np.array_equal(st["qvel"], want["qvel"]), c["name"]
        if c["name"].startswith("norm_"):
            print(f"\nEDGE {c['name']}: the device root quaternion has norm {np.linalg.norm(st['qpos'][3:7])!r}, the root body's world quaternion {np.linalg.norm(st['xquat'][1])!r}")
        if "unset" in c["claims"]:
            assert st["xquat"][1, 0] == 0.0, f"{c['name']}: the forward pass left w = {st['xquat'][1, 0]!r} on the root body"
        b = C.obs_branches(st, w)
        assert b["unset"] == ("unset" in c["claims"]) and min(b["hq_crq"], b["hq_rootq"], b["hq_trq"]) >= 1e-3
        for claim, key in (("z_neg", "z_neg"), ("w_neg", "w_neg")):  # the device state is on the claimed side too
            assert (claim in c["claims"]) == b[key] or not c["name"].startswith("yaw"), (c["name"], claim)
        ref, bar, excluded = C.obs_reference(kind, st, w, 0, beta[where[i, 0]], seed=i)
        assert not excluded, c["name"]
        worst.check(gobs[env], ref, bar, c["name"])
    sb.close()
    worst.report()


@pytest.mark.parametrize("kind", C.OBS_KINDS)
def test_reset_observation_at_crafted_states(model, ctrl, obs_table, kind):
    _reset_observation(model, ctrl, obs_table, kind)


# ----------------------------------------------------------------------------------------------------------- 2. reward / termination, two passes
def _walk_windows(humanoid, walk, n, length=3):
    return [C.frames_of_rows(humanoid, walk[i:i + length]) for i in range(n)]


def _action(kind, explicit, n, dim, seed):
    if explicit:
        return C.explicit_action(n, dim, seed)
    return np.random.default_rng(seed).normal(scale=0.003 if kind == "ball" else 0.1, size=(n, dim))


@pytest.mark.parametrize("rv,okind,thresh,w_vf", C.REWARD_FLAVOURS)
def test_reward_and_termination_at_crafted_targets(model, ctrl, humanoid, walk, rv, okind, thresh, w_vf):
    import torch
    from uhc_amd import sim as S
    ball, expl = okind == "ball", rv in (1, 3)
    w = C.reward_weights(rv, w_vf)
    n = len(C.REWARD_CASES)
    sb, eb, ctrl = _make(model, okind, n, rv=rv, ctrl=ctrl, explicit=expl, reward_weights=w, body_diff_thresh=thresh)
    from uhc_amd.smpllib.smpl_mujoco import SMPLConverter
    jw = SMPLConverter(model, model).get_new_diff_weight()
    dt = model.timestep * 15
    wins = _walk_windows(humanoid, walk, n)
    ids = np.arange(n, dtype=np.int32)
    act = _action(okind, expl, n, ctrl.action_dim, 4)
    d_act = torch.from_numpy(act).cuda()
    kw = {} if expl else dict(vf_dim=0 if ball else 6, ball=ball)
    # pass 1: where does one control step take every env
    bank = C.assemble_bank(wins)
    _set_bank(eb, bank)
    _assign_reset(eb, ids, bank[2])
    prev = sb.field(S.F_QPOS).cpu().numpy().copy()
    eb.step(d_act, None)
    sb.sync()
    rb1 = _readback(sb)
    # pass 2: the same step against frame-1 records rewritten relative to that state (qpos and qvel slots, which the physics reads, untouched)
    keep = [x.copy() for x in wins]
    for e, case in enumerate(C.REWARD_CASES):
        C.craft_reward_record(wins[e][1], case, _state(rb1, e), prev[e], dt, jw, ball, seed=100 + e)
        assert np.array_equal(wins[e][1, :151], keep[e][1, :151]) and np.array_equal(wins[e][[0, 2]], keep[e][[0, 2]])
    bank = C.assemble_bank(wins)
    _set_bank(eb, bank)
    _assign_reset(eb, ids, bank[2])
    assert np.array_equal(sb.field(S.F_QPOS).cpu().numpy(), prev)
    eb.step(d_act, None)
    sb.sync()
    rb = _readback(sb)
    assert np.array_equal(rb["qpos"], rb1["qpos"]) and np.array_equal(rb["qvel"], rb1["qvel"])  # the PD target lives in the record's qpos: bit-identical
    g = {k: eb.field(f).cpu().numpy() for k, f in dict(r=S.E_REWARD, parts=S.E_REWARD_PARTS, bd=S.E_BODY_DIFF, fail=S.E_FAIL, end=S.E_END, done=S.E_DONE,
                                                       pct=S.E_PERCENT, t=S.E_CUR_T, obs=S.E_OBS, ep=S.E_EPISODE).items()}
    sim_fail = sb.field(S.F_FAIL).cpu().numpy()
    beta = C.clip_beta_rows()
    worst, worst_ill, worst_obs = _Worst(f"reward_v {rv} ({okind})"), _Worst(f"reward_v {rv} ({okind}) next to acos(-1)"), _Worst(f"next obs {okind} after reward_v {rv}")
    for e, case in enumerate(C.REWARD_CASES):
        st = _state(rb, e)
        ref, bar, excluded = C.reward_reference(rv, st, prev[e], act[e], wins[e], 1, dt, jw, w, thresh, seed=e, check_side=case != "bd_eq0.5", **kw)
        assert not excluded, case
        if case == "bd_eq0.5":  # exact on both sides: the distance IS 0.5, and 0.5 > 0.5 is no failure
            assert ref[-1] == 0.5 and g["bd"][e] == 0.5 and int(g["fail"][e]) == int(0.5 > thresh) and not sim_fail[e]
        (worst_ill if case in ("quat_neg", "quat_mixed", "quat_rot359.9") else worst).check(np.r_[g["r"][e], g["parts"][e], g["bd"][e]], ref, bar, case)
        fail = bool(sim_fail[e]) or bool(ref[-1] > thresh)
        if case.startswith("bd_") and case != "bd_eq0.5":
            t_, above = float(case[3:-1]), case.endswith("+")
            assert (ref[-1] > t_) == above and abs(ref[-1] - t_) < 2 * C.BD_MARGIN and not sim_fail[e]
        assert (int(g["fail"][e]), int(g["end"][e]), int(g["done"][e])) == (int(fail), 0, int(fail)), case
        assert g["t"][e] == 1 and g["pct"][e] == 0.5
        assert g["ep"][0, e] == 1.0 and g["ep"][1, e] == g["r"][e]
        oref, obar, oex = C.obs_reference(okind, st, wins[e], 1, beta[bank[2][e, 0]], seed=e)
        assert not oex
        worst_obs.check(g["obs"][e], oref, obar, case)
    for x in (worst, worst_ill, worst_obs):
        x.report()
    sb.close()


# ----------------------------------------------------------------------------------------------------------- trail steps, episode length, accounting
@pytest.mark.parametrize("rv,trail,episode_len,steps", [(1, 3, 100000, 5), (3, 3, 100000, 5), (0, 3, 100000, 5), (0, 0, 2, 2)],
                         ids=["explicit-trail3", "explicit_mul-trail3", "implicit-trail3", "episode_len2"])
def test_trail_steps_episode_length_and_accounting(model, ctrl, humanoid, walk, rv, trail, episode_len, steps):
    import torch
    from uhc_amd import sim as S
    from uhc_amd.smpllib.smpl_mujoco import SMPLConverter
    expl = rv in (1, 3)
    w = dict(C.REWARD_W, k_p=2.0)
    END_REWARD = 2.5
    lens = [3, 3, 20] if trail else [20, 20, 20]
    n = len(lens)
    sb, eb, ctrl = _make(model, 2, n, rv=rv, ctrl=ctrl, explicit=expl, reward_weights=w, env_expert_trail_steps=trail, env_episode_len=episode_len)
    eb.set_end_reward(END_REWARD)
    jw = SMPLConverter(model, model).get_new_diff_weight()
    dt = model.timestep * 15
    wins = [C.frames_of_rows(humanoid, walk[s:s + L]) for s, L in zip((0, 7, 3), lens)]
    b0, bn = C.FR["bangvel"]
    for x in wins:  # a large expert angular velocity on the last frame: a reward that keeps reading it past the clip end shows
        x[-1, b0:b0 + bn] = 5.0 * np.where(np.arange(bn) % 2 == 0, 1.0, -1.0)
    bank = C.assemble_bank(wins)
    _set_bank(eb, bank)
    ids = np.arange(n, dtype=np.int32)
    _assign_reset(eb, ids, bank[2])
    # env 1 has a window queued behind its current one: the snapshot's fifth row
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32)  # noqa: E731
    eb.set_next(i32(1), i32(int(bank[2][2, 0])), i32(int(bank[2][2, 1])), i32(10), None)
    rng = np.random.default_rng(9)
    kw = {} if expl else dict(vf_dim=6)
    ret, ret_bar = np.zeros(n), np.zeros(n)
    worst = _Worst(f"reward_v {rv} trail {trail} episode_len {episode_len}")
    sched = [C.episode_schedule(L, trail, episode_len, steps) for L in lens]
    for k in range(steps):
        act = C.explicit_action(n, ctrl.action_dim, 30 + k) if expl else rng.normal(scale=0.1, size=(n, ctrl.action_dim))
        prev = sb.field(S.F_QPOS).cpu().numpy().copy()
        eb.step(torch.from_numpy(act).cuda(), None)
        sb.sync()
        rb = _readback(sb)
        g = {k_: eb.field(f).cpu().numpy() for k_, f in dict(r=S.E_REWARD, parts=S.E_REWARD_PARTS, bd=S.E_BODY_DIFF, fail=S.E_FAIL, end=S.E_END, done=S.E_DONE,
                                                             pct=S.E_PERCENT, t=S.E_CUR_T, ep=S.E_EPISODE).items()}
        sim_fail = sb.field(S.F_FAIL).cpu().numpy()
        for e in range(n):
            cur_t, ind, past, end, pct = sched[e][k]
            ref, bar, excluded = C.reward_reference(rv, _state(rb, e), prev[e], act[e], wins[e], cur_t, dt, jw, w, 0.5, seed=10 * k + e, **kw)
            assert not excluded
            worst.check(np.r_[g["r"][e], g["parts"][e], g["bd"][e]], ref, bar, f"env {e} step {cur_t}")
            fail = bool(sim_fail[e]) or bool(ref[-1] > 0.5)
            assert not fail
            assert (int(g["fail"][e]), int(g["end"][e]), int(g["done"][e]), int(g["t"][e])) == (0, int(end), int(end), cur_t), (e, cur_t)
            assert g["pct"][e] == pytest.approx(pct, abs=1e-15)
            ret[e] += ref[0] + (END_REWARD if end else 0.0)
            ret_bar[e] += bar[0] + 1e-14
            assert g["ep"][0, e] == cur_t and abs(g["ep"][1, e] - ret[e]) <= ret_bar[e]  # the end reward enters on the end step only
    assert [s[-1][3] for s in sched] == ([True, True, False] if trail else [True, True, True])
    if trail:
        assert sched[0][-1][4] == 2.5 and [s[2] for s in sched[0]] == [False, False, True, True, True]
    done = eb.field(S.E_DONE).cpu().numpy().copy()
    pct = eb.field(S.E_PERCENT).cpu().numpy().copy()
    ep = eb.field(S.E_EPISODE).cpu().numpy().copy()
    eb.auto_reset()
    sb.sync()
    snap = eb.field(S.E_SNAPSHOT).cpu().numpy()
    assert snap[0].tolist() == done.tolist() and np.array_equal(snap[1], ep[0]) and np.array_equal(snap[2], ep[1]) and np.array_equal(snap[3], pct)
    assert snap[4].tolist() == [0.0, 1.0, 0.0] and eb.field(S.E_CONSUMED).cpu().numpy().tolist() == [0, 1, 0]
    ep2, t2 = eb.field(S.E_EPISODE).cpu().numpy(), eb.field(S.E_CUR_T).cpu().numpy()
    for e in range(n):
        assert (ep2[:, e] == 0.0).all() and t2[e] == 0 if done[e] else np.array_equal(ep2[:, e], ep[:, e]) and t2[e] == steps
    worst.report()
    sb.close()
