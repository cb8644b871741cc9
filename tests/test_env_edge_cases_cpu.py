"""The case tables of tests/env_edge_cases.py, without a GPU: on stand-in states (the crafted frame's own qpos_fk output as the "device"
state) every named case reaches the oracle branch it claims, no case sits so close to a switch that a one-step move of the inputs
changes sides (zero exclusions), and the tolerance derived from the oracle stays tight where the arithmetic is well conditioned."""
import math
import os

import numpy as np
import pytest

from tests import env_edge_cases as C

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def humanoid(model):
    from uhc_amd.smpllib.torch_smpl_humanoid import Humanoid
    return Humanoid(model=model)


@pytest.fixture(scope="module")
def table(humanoid):
    cases = C.obs_cases()
    return cases, C.obs_windows(humanoid, cases)


def test_observation_cases_reach_their_branches(table):
    cases, wins = table
    seen = set()
    for c, w in zip(cases, wins):
        b = C.obs_branches(C.stand_in_state(w), w)
        assert min(b["hq_crq"], b["hq_rootq"], b["hq_trq"]) >= 1e-3, c["name"]  # the reference is NaN at 0
        assert b["unset"] == ("unset" in c["claims"]), c["name"]
        assert w.shape[0] == c["rows"].shape[0] and b["target_is_state"] == ("len1" in c["claims"])
        for claim in c["claims"]:
            seen.add(claim)
            ok = {"z_neg": b["z_neg"] and b["z_neg_root"], "w_neg": b["w_neg"], "unset": b["unset"], "len1": w.shape[0] == 1,
                  "acos_raw_above_pi": b["acos_raw"] > math.pi, "acos_raw_below_minus_pi": b["acos_raw"] < -math.pi,
                  "atan_raw_above_pi": b["atan_raw"] > math.pi, "atan_raw_below_minus_pi": b["atan_raw"] < -math.pi,
                  "hq_small_crq": b["hq_crq"] < 3e-3, "hq_small_rootq": b["hq_rootq"] < 3e-3,
                  "v3_all_clamped": all(i >= w.shape[0] - 1 for i in (1, 5, 9)), "v3_last_clamped": b["clamped"] == (False, False, True),
                  "v3_none_clamped": b["clamped"] == (False, False, False)}[claim]
            assert ok, (c["name"], claim, b)
    assert seen == {"z_neg", "w_neg", "unset", "len1", "acos_raw_above_pi", "acos_raw_below_minus_pi", "atan_raw_above_pi", "atan_raw_below_minus_pi",
                    "hq_small_crq", "hq_small_rootq", "v3_all_clamped", "v3_last_clamped", "v3_none_clamped"}
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names) and 36 <= len(names) < 64
    # both quadrant signs of w and z, q and -q of every yaw
    assert sum("z_neg" in c["claims"] for c in cases) >= 8 and sum("w_neg" in c["claims"] for c in cases) >= 8


def test_joint_and_velocity_extremes_are_in_the_table(table, model):
    cases, wins = table
    lo, hi = np.asarray(model.jnt_range)[1:, 0], np.asarray(model.jnt_range)[1:, 1]
    j = {c["name"]: c for c in cases}
    assert (j["joints_hi"]["rows"][0, 7:] == hi).all() and (j["joints_lo"]["rows"][0, 7:] == lo).all() and (hi >= 3.14159).all()
    assert (np.abs(j["joints_alt_pi"]["rows"][:, 7:]) == math.pi).all()
    beyond = j["joints_beyond"]["rows"][:, 7:]
    assert ((beyond > hi + 0.4) | (beyond < lo - 0.4)).all()
    for n in ("joints_hi", "joints_lo", "joints_alt_pi", "joints_beyond"):
        w = wins[[c["name"] for c in cases].index(n)]
        assert (np.abs(C.stand_in_state(w)["qvel"][6:]) == 50.0).all()  # (qpos_fk clips its own velocities to +-10: the slot was overwritten)
    for n, s in (("norm_1.001", 1.001), ("norm_0.999", 0.999)):
        assert np.linalg.norm(j[n]["rows"][0, 3:7]) == pytest.approx(s, abs=1e-12)


def test_bank_addressing(table):
    cases, wins = table
    frames, clip_start, where = C.assemble_bank(wins)
    assert len(clip_start) == C.N_CLIPS >= 5 and (np.diff(clip_start) > 0).all() and clip_start[-1] > 200
    assert len(set(where[:, 0])) == C.N_CLIPS and where[:, 1].min() >= 5
    owned = np.zeros(frames.shape[0], dtype=bool)
    for w, (c, s, n) in zip(wins, where):
        a = clip_start[c] + s
        assert np.array_equal(frames[a:a + n], w) and not owned[a:a + n].any()
        owned[a:a + n] = True
    assert (frames[~owned] == C.POISON).all() and not owned[-1]  # one frame past any window is another window's or poison, never outside the bank
    ids = C.env_ids_for(len(cases), 48)
    assert len(set(ids)) == len(cases) < 48 and not np.array_equal(ids, np.sort(ids))
    beta = C.clip_beta_rows()
    assert beta.shape == (C.N_CLIPS, 17) and len({tuple(r) for r in beta}) == C.N_CLIPS


@pytest.mark.parametrize("kind", C.OBS_KINDS)
def test_observation_table_has_no_exclusions_and_tight_bars(table, kind):
    cases, wins = table
    beta = C.clip_beta_rows()
    excluded, worst = [], {}
    for i, (c, w) in enumerate(zip(cases, wins)):
        st = C.stand_in_state(w, ball=kind == "ball")
        ref, bar, ex = C.obs_reference(kind, st, w, 0, beta[i % C.N_CLIPS], seed=i)
        assert ref.shape == (C.OBS_DIM[kind],)
        assert np.isfinite(ref).all() and np.isfinite(bar).all(), c["name"]
        if ex:
            excluded.append(c["name"])
        worst[c["name"]] = bar.max()
    assert excluded == []
    print(f"obs {kind}: largest bar {max(worst.values()):.2e} ({max(worst, key=worst.get)}), median case {np.median(list(worst.values())):.2e}")
    # well-conditioned cases (mid-quadrant yaw, unit quaternions, moderate velocities) stay below the 1e-11 reset bar of test_gpu_env.py
    for n in ("yaw+0.7000q", "yaw-2.2000-q", "len3", "wrap_acos_hi", "wrap_atan_lo"):
        assert worst[n] < 1e-11, (n, worst[n])


def _walk_window(humanoid, start, n=3):
    e = np.load(os.path.join(G, "g3_qpos_fk.npz"))["f_qpos"]
    return C.frames_of_rows(humanoid, e[start:start + n])


@pytest.mark.parametrize("rv,okind,thresh,w_vf", C.REWARD_FLAVOURS)
def test_reward_cases_reach_their_branches(humanoid, model, rv, okind, thresh, w_vf):
    from oracle import env_oracle as E
    from uhc_amd.smpllib.smpl_mujoco import SMPLConverter
    from uhc_amd.utils.math_utils import multi_quat_diff
    jw = SMPLConverter(model, model).get_new_diff_weight()
    ball = okind == "ball"
    dt = model.timestep * 15
    w = C.reward_weights(rv, w_vf)
    expl = rv in (1, 3)
    act = C.explicit_action(len(C.REWARD_CASES), 69 + 216 + 30, 4) if expl else np.random.default_rng(4).normal(scale=0.1, size=(len(C.REWARD_CASES), 105))
    worst = {}
    for i, case in enumerate(C.REWARD_CASES):
        win = _walk_window(humanoid, i)
        st = C.stand_in_state(win, ball=ball, frame=1)
        prev = C.stand_in_state(win, ball=ball, frame=0)["qpos"]
        C.craft_reward_record(win[1], case, st, prev, dt, jw, ball, seed=100 + i)
        kw = {} if expl else dict(vf_dim=0 if ball else 6, ball=ball)
        # (bd_eq0.5 sits ON the switch by construction, in exact arithmetic: it is a comparison of exact values, not one under a tolerance, and has no side to keep)
        ref, bar, ex = C.reward_reference(rv, st, prev, act[i], win, 1, dt, jw, w, thresh, seed=i, check_side=case != "bd_eq0.5", **kw)
        assert not ex, case
        if case == "bd_eq0.5":
            assert ref[-1] == 0.5 and not ref[-1] > 0.5
            continue
        n_parts = 6 if rv >= 4 else (4 if ball else 5)  # (no residual force on the ball env: its fifth part is 0)
        assert np.isfinite(ref).all() and (ref[1:1 + n_parts] > 1e-9).all(), (case, ref)  # no term underflows: a wrong one shows
        worst[case] = bar[:7].max()
        ex_d = C.expert_of_window(win)
        if case.startswith("bd_") :
            t, above = float(case[3:-1]), case.endswith("+")
            assert abs(ref[-1] - (t + (C.BD_MARGIN if above else -C.BD_MARGIN))) < 1e-12 and (ref[-1] > t) == above and bar[-1] < 1e-13
        if case.startswith("quat_"):
            cur = E.get_body_quat_ball(st["qpos"]) if ball else E.get_body_quat(st["qpos"])
            dq0 = multi_quat_diff(cur, ex_d["bquat"][1])[::4]
            wq0 = multi_quat_diff(st["xquat"][1:].ravel(), ex_d["wbquat"][1])[::4]
            k = case[5:]
            if k == "exact":
                assert np.abs(dq0 - 1).max() < 1e-15 and np.abs(wq0 - 1).max() < 1e-15
            if k == "neg":
                assert np.abs(dq0 + 1).max() < 1e-15 and np.arccos(np.clip(dq0, -1, 1)).min() > 3.14159
            if k == "scaled":
                assert np.abs(dq0 - 1 / 1.001).max() < 1e-14
            if k == "rot179.9":
                assert np.abs(dq0 - math.cos(math.radians(89.95))).max() < 1e-14
            if k == "mixed":
                assert dq0.min() < -0.99 and dq0.max() > 0.9999 and 0 < np.abs(dq0).min() < 1e-3
    # acos next to -1 (the negated target, 359.9 degrees) is ill conditioned -- d acos = d x / sqrt(1 - x^2), 1.5e-8 for one rounding of x --: everywhere else the bar
    # stays below the reset bar of test_gpu_env.py
    ill = ("quat_neg", "quat_mixed", "quat_rot359.9")
    well = max(v for k, v in worst.items() if k not in ill)
    print(f"reward_v {rv} ({okind}): largest bar of reward and parts {well:.2e}; next to acos(-1) {max(worst[k] for k in ill):.2e}")
    assert well < 1e-11, worst
    if expl:  # every one of a body's nine residual entries differs, so a wrong `k % 9 >= 3` selection changes the sum
        a = act[0][69:69 + 216].reshape(24, 9)
        assert all(len(set(np.abs(r))) == 9 for r in a) and (a[:, :3] != 0).all()


def test_episode_schedules():
    s = C.episode_schedule(3, 3, 100000, 5)
    assert [x[1] for x in s] == [1, 2, 2, 2, 2]                 # the expert index clamps
    assert [x[2] for x in s] == [False, False, True, True, True]  # `past`: the explicit rewards' expert velocity is zero from here
    assert [x[3] for x in s] == [False, False, False, False, True] and s[-1][4] == 2.5  # three steps after the window's end; percent beyond 1
    s = C.episode_schedule(30, 0, 2, 2)
    assert [x[3] for x in s] == [False, True] and not s[1][2]   # env_episode_len ends it, not the window
