"""Friction-loss rows, joint springs and slide joints on the device, on every tier, against the free-running CPU oracle.

The cases, their oracle trajectories and their bars are tests/passive_cases.py's; tests/test_passives_cpu.py proves on the oracle alone that every case reaches the
branches it is named for, so nothing is skipped or filtered here: every env of every case is compared at every control step.  No UHC_F_REDO word is handed to the oracle
(as in test_oracle_decides_its_own_solver): friction-loss rows send BOTH sides to the sweeps, from the warm start, and the two must agree on their own.

What a step with friction-loss rows reports (the sentence in include/uhc_amd.h at UHC_F_REDO, asserted below): the fast tier sweeps without saying so -- its word stays 0;
at solver 1 the general tier, the large tier and tier 4 report SWEPT | WHY_FRICTION and the swept bit of every substep they computed, tier 4 without PRIMAL; at solver 0
the general and the large tier report SWEPT and the substep bits without a reason, tier 4 reports neither."""
import os

import numpy as np
import pytest

from tests import passive_cases as P
from uhc_amd.sim import (REDO_DROPPED, REDO_GENERAL, REDO_LARGE, REDO_PRIMAL, REDO_PRIMAL_CAP, REDO_SWEPT, REDO_SWEPT_SUBSTEP0, REDO_WHY_FRICTION, REDO_WHY_NOCONV,
                         REDO_WHY_PIVOT, REDO_WINDOWED, WHY_CONTACTS, WHY_FAST_SHIFT, WHY_FIELD, WHY_GENERAL_SHIFT, WHY_LARGE_SHIFT, WHY_ROWS, WHY_SOLVER, WHY_SUBSTEP_SHIFT)

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["fast", "general"], autouse=True)
def kernel_path(request):
    """As in test_gpu_physics.py: every test runs on the tier chain that starts with the fast tier and on the one that starts with the general tier."""
    old = os.environ.get("UHC_FORCE_GENERAL")
    os.environ["UHC_FORCE_GENERAL"] = "1" if request.param == "general" else "0"
    yield request.param
    if old is None:
        os.environ.pop("UHC_FORCE_GENERAL", None)
    else:
        os.environ["UHC_FORCE_GENERAL"] = old


FIELDS = dict(xpos="F_XPOS", xquat="F_XQUAT", xipos="F_XIPOS", qM="F_QM", qfrc_bias="F_QFRC_BIAS", qacc="F_QACC")


def _batch(c, envs=None):
    """The case's envs (or the subset `envs`) as a device batch at the case's state."""
    import torch
    from uhc_amd import sim as S
    envs = list(range(c.n_env)) if envs is None else list(envs)
    used = sorted({c.env_model[e] for e in envs})
    b = S.SimBatch([c.models[k] for k in used], c.ctrl, len(envs), env_model=[used.index(c.env_model[e]) for e in envs] if len(used) > 1 else None)
    b.set_state(torch.from_numpy(c.qpos[envs].copy()), torch.from_numpy(c.qvel[envs].copy()))
    b.sync()
    return b


def _get(b, *names):
    from uhc_amd import sim as S
    return [b.field(getattr(S, n)).cpu().numpy().copy() for n in names]


def _run(c, envs=None):
    """The case on the device: per control step qpos, qvel, ncon, nefc and the control words of every env."""
    import torch
    envs = list(range(c.n_env)) if envs is None else list(envs)
    b = _batch(c, envs)
    first = dict(zip(("qacc", "ncon", "nefc"), _get(b, "F_QACC", "F_NCON", "F_NEFC")))
    tb = torch.from_numpy(c.target[envs].copy()).cuda()
    out = dict(first=first, qpos=[], qvel=[], ncon=[], nefc=[], redo=[], why=[])
    for t in range(c.steps):
        b.simulate(torch.from_numpy(c.act[t][envs].copy()).cuda(), tb)
        b.sync()
        for k, v in zip(("qpos", "qvel", "ncon", "nefc", "redo", "why"), _get(b, "F_QPOS", "F_QVEL", "F_NCON", "F_NEFC", "F_REDO", "F_HANDON_WHY")):
            out[k].append(v)
    out["overflow"], out["fail"] = _get(b, "F_EFC_OVERFLOW", "F_FAIL")
    b.close()
    return {k: (np.stack(v) if isinstance(v, list) else v) for k, v in out.items()}


def _compare(name, dev, envs=None):
    """Every env at every control step against the oracle's own trajectory: counts equal, qpos / qvel within the case's bars.  The figures are printed before they are asserted."""
    r = P.reference(name)
    c = r["case"]
    envs = list(range(c.n_env)) if envs is None else list(envs)
    worst = dict(qpos=0.0, qvel=0.0, qacc=0.0)
    counts_ok = True
    for k, e in enumerate(envs):
        run = r["runs"][e]
        worst["qacc"] = max(worst["qacc"], float(np.abs(dev["first"]["qacc"][k] - run["first"]["qacc"]).max()))
        worst["qpos"] = max(worst["qpos"], float(np.abs(dev["qpos"][:, k] - run["qpos"]).max()))
        worst["qvel"] = max(worst["qvel"], float(np.abs(dev["qvel"][:, k] - run["qvel"]).max()))
        counts_ok = counts_ok and dev["first"]["nefc"][k] == run["nefc"][0] and dev["first"]["ncon"][k] == run["ncon"][0] and \
            np.array_equal(dev["nefc"][:, k], run["nefc"][1:]) and np.array_equal(dev["ncon"][:, k], run["ncon"][1:])
    print(f"PASSIVES {name:30s} " + " ".join(f"{q} dev {worst[q]:.2e} bar {r['bars'][q]:.2e}" for q in ("qpos", "qvel", "qacc")) + f" counts {'equal' if counts_ok else 'DIFFER'}")
    assert counts_ok, "ncon / nefc differ from the oracle's at some step"
    for q in ("qpos", "qvel", "qacc"):
        assert worst[q] <= r["bars"][q], (name, q, worst[q], r["bars"][q])
    assert not dev["fail"].any() and not dev["overflow"].any()


def _why(word, shift):
    return (int(word) >> shift) & WHY_FIELD


def _check_words(c, dev, kernel_path, solver, friction):
    """The control words of every env after every step, by the tier the case is named for.  friction[k]: env k has friction-loss rows."""
    n_sub = int(c.ctrl.n_substeps)
    all_substeps = sum(REDO_SWEPT_SUBSTEP0 << k for k in range(n_sub))
    for t in range(dev["redo"].shape[0]):
        for k in range(dev["redo"].shape[1]):
            w, why = int(dev["redo"][t, k]), int(dev["why"][t, k])
            assert not w & (REDO_WHY_NOCONV | REDO_WHY_PIVOT | REDO_DROPPED | REDO_WINDOWED | REDO_PRIMAL | REDO_PRIMAL_CAP), (c.name, t, k, hex(w))
            for shift in (WHY_FAST_SHIFT, WHY_GENERAL_SHIFT, WHY_LARGE_SHIFT):
                assert not _why(why, shift) & WHY_SOLVER and not _why(why, shift) & ~(WHY_ROWS | WHY_CONTACTS), (c.name, t, k, hex(why))
            if c.tier == "fast" and kernel_path == "fast":
                assert w == 0 and why == 0, (c.name, t, k, hex(w), hex(why))  # the fast tier sweeps its friction-loss rows without a word
                continue
            assert w & REDO_GENERAL, (c.name, t, k, hex(w))
            if kernel_path == "fast":  # the fast tier handed the env on: by rows or contacts
                assert _why(why, WHY_FAST_SHIFT) & (WHY_ROWS | WHY_CONTACTS), (c.name, t, k, hex(why))
            if c.tier in ("fast", "general"):
                assert not w & REDO_LARGE and _why(why, WHY_GENERAL_SHIFT) == 0 and _why(why, WHY_LARGE_SHIFT) == 0, (c.name, t, k, hex(w), hex(why))
            if c.tier in ("large", "tier4"):
                assert w & REDO_LARGE and _why(why, WHY_GENERAL_SHIFT) & (WHY_ROWS | WHY_CONTACTS), (c.name, t, k, hex(w), hex(why))
            assert (_why(why, WHY_LARGE_SHIFT) != 0) == (c.tier == "tier4"), (c.name, t, k, hex(why))
            if solver == 1:
                if friction[k]:
                    assert w & REDO_SWEPT and w & REDO_WHY_FRICTION and w & all_substeps == all_substeps, (c.name, t, k, hex(w))
                else:  # an env without friction-loss rows is solved exactly, whatever its neighbours in the batch are
                    assert not w & (REDO_SWEPT | REDO_WHY_FRICTION | all_substeps), (c.name, t, k, hex(w))
            elif c.tier == "tier4":  # solver 0 is no fallback: tier 4 says nothing ...
                assert not w & (REDO_SWEPT | REDO_WHY_FRICTION | all_substeps), (c.name, t, k, hex(w))
            else:  # ... the general and the large tier report their sweeps, without a reason
                assert w & REDO_SWEPT and not w & REDO_WHY_FRICTION and w & all_substeps == all_substeps, (c.name, t, k, hex(w))


# ------------------------------------------------------------------ the slider: forward fields
@pytest.mark.parametrize("springs", [False, True], ids=["plain", "springs"])
def test_slider_forward_fields_match_oracle(springs, kernel_path):
    """slide - hinge - slide at 16 seeded states, slide positions on both sides of qpos0 and four beyond the rail's limit; with springs whose rest position is not qpos0,
    and without."""
    r = P.forward_reference(springs)
    c = r["case"]
    b = _batch(c)
    g = dict(zip(list(FIELDS) + ["ncon", "nefc"], _get(b, *FIELDS.values(), "F_NCON", "F_NEFC")))
    b.close()
    worst = {k: max(float(np.abs(g[k][e] - run["first"][k]).max()) for e, run in enumerate(r["runs"])) for k in FIELDS}
    print(f"PASSIVES {c.name:30s} " + " ".join(f"{k} dev {worst[k]:.2e} bar {r['bars'][k]:.2e}" for k in FIELDS))
    for e, run in enumerate(r["runs"]):
        assert g["ncon"][e] == 0 and g["nefc"][e] == run["nefc"][0]
    for k in FIELDS:
        assert worst[k] <= r["bars"][k], (k, worst[k], r["bars"][k])


# ------------------------------------------------------------------ the slider: trajectories, friction-bound edges
@pytest.mark.parametrize("name", ["slider_spring", "slider_friction", "slider_spring_friction_limit", "slider_friction_limit_two_sweeps", "friction_bound_tiny", "friction_bound_half", "friction_bound_huge"])
def test_slider_trajectory_matches_free_running_oracle(name, kernel_path):
    """Spring only, friction loss only, spring + friction loss + the rail's limit; and the friction bound's edges on a state and its mirror image -- 1e-9 (no friction to
    speak of: always saturated), 0.5, 1e9 (an equality: never saturated).  Seeded motor torques, three substeps per control step.  The case capped at two sweeps stops far
    from the optimum, where the forces depend on the order of the rows: friction-loss rows, then limits, as the oracle (and MuJoCo) enumerates them."""
    c = P.case(name)
    dev = _run(c)
    _compare(name, dev)
    _check_words(c, dev, kernel_path, 1, [bool((np.asarray(c.model_of(e).dof_frictionloss) > 0).any()) for e in range(c.n_env)])


# ------------------------------------------------------------------ every tier
@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("n_seg", [s[0] for s in P.CATERPILLARS])
def test_friction_loss_on_every_tier(n_seg, solver, kernel_path):
    """The caterpillar with friction loss on its hinge dofs and springs on its hinges: 4 segments stay in the fast tier, 6 in the general, 12 in the large, 27 in tier 4."""
    name = f"caterpillar{n_seg}_solver{solver}"
    c = P.case(name)
    dev = _run(c)
    _compare(name, dev)
    _check_words(c, dev, kernel_path, solver, [True] * c.n_env)


def test_rows_beyond_the_large_tier_are_dropped_and_flagged_without_tier_4(kernel_path, monkeypatch):
    """UHC_TIERS=3: the large tier is the last one, and the 27-segment animal's rows beyond 256 are dropped.  That is no longer the oracle's problem: the test asserts the
    flags, and that the step stays finite and bounded."""
    monkeypatch.setenv("UHC_TIERS", "3")
    c = P.case("caterpillar27_solver1")
    dev = _run(c)
    assert (dev["redo"] & REDO_DROPPED).all() and (dev["redo"] & REDO_LARGE).all() and not (dev["redo"] & (REDO_PRIMAL | REDO_PRIMAL_CAP)).any(), [hex(int(w)) for w in dev["redo"].ravel()]
    assert (dev["overflow"] > 0).all() and not dev["fail"].any()
    assert (dev["nefc"] <= P.LARGE_ROWS).all()
    assert np.isfinite(dev["qpos"]).all() and np.isfinite(dev["qvel"]).all()
    assert np.abs(dev["qpos"] - c.qpos[None]).max() < 0.05 and np.abs(dev["qvel"]).max() < 5.0, (np.abs(dev["qpos"] - c.qpos[None]).max(), np.abs(dev["qvel"]).max())


# ------------------------------------------------------------------ a batch of envs with and without friction-loss rows
def test_mixed_batch_keeps_friction_free_envs_on_the_exact_path(kernel_path):
    """Two models of one topology, dof_frictionloss all zero against positive, interleaved over 8 envs.  Whether a solve has friction-loss rows is decided per env: the
    friction-free envs are solved exactly (no SWEPT in any tier), and every env equals, bit for bit, the same env in a batch of its own model alone."""
    c = P.case("mixed_batch")
    friction = [bool((np.asarray(c.model_of(e).dof_frictionloss) > 0).any()) for e in range(c.n_env)]
    assert friction == [False, True] * 4
    dev = _run(c)
    _compare("mixed_batch", dev)
    _check_words(c, dev, kernel_path, 1, friction)
    for k in (0, 1):
        envs = [e for e in range(c.n_env) if c.env_model[e] == k]
        alone = _run(c, envs)
        for q in ("qpos", "qvel", "redo", "nefc"):
            np.testing.assert_array_equal(alone[q], dev[q][:, envs], err_msg=f"model {k}: {q} in the mixed batch and alone")
        np.testing.assert_array_equal(alone["first"]["qacc"], dev["first"]["qacc"][envs])


# ------------------------------------------------------------------ the humanoid the configs describe
def test_humanoid_with_friction_loss_and_springs_on_its_hinges(kernel_path):
    """The headline model with friction loss 1.0 and stiffness 5 on its 69 hinge dofs (robot.joint_params of the reference's configs): more than 64 rows before the first
    contact, so no step of it is the fast tier's -- every one takes the sweep path of the general (or large) tier.  Ten control steps of stable-PD actions."""
    c = P.case("humanoid_passives")
    dev = _run(c)
    assert (dev["first"]["nefc"] >= 69).all()
    _compare("humanoid_passives", dev)
    n_sub = int(c.ctrl.n_substeps)
    every = sum(REDO_SWEPT_SUBSTEP0 << k for k in range(n_sub))
    for w, why in zip(dev["redo"].ravel(), dev["why"].ravel()):
        w, why = int(w), int(why)
        assert w & REDO_GENERAL and w & REDO_SWEPT and w & REDO_WHY_FRICTION, hex(w)
        # (the swept bits are those of the substeps the tier that FINISHED the step computed: an env whose rows outgrow the general tier in substep k is handed to
        #  the large tier there, and its word holds substeps k and later)
        start = _why(why, WHY_SUBSTEP_SHIFT) if w & REDO_LARGE else 0
        assert w & every == sum(REDO_SWEPT_SUBSTEP0 << k for k in range(start, n_sub)), (hex(w), hex(why))
        assert not w & (REDO_WHY_NOCONV | REDO_WHY_PIVOT | REDO_DROPPED | REDO_PRIMAL | REDO_PRIMAL_CAP), hex(w)
        assert not any(_why(why, s) & WHY_SOLVER for s in (WHY_FAST_SHIFT, WHY_GENERAL_SHIFT, WHY_LARGE_SHIFT)), hex(why)
        if kernel_path == "fast":
            assert _why(why, WHY_FAST_SHIFT) & WHY_ROWS, hex(why)


# ------------------------------------------------------------------ springs are a hinge's and a slide's
def test_stiffness_on_ball_and_free_joints_changes_nothing_on_the_device(model, standing, kernel_path):
    """The ball-joint humanoid of test_gpu_ball.py, in free flight, with a stiffness on every ball joint and on the free root (and a rest position that is not qpos0): bit for
    bit the run without (tests/test_passives_cpu.py shows the same of the oracle)."""
    import dataclasses
    import torch
    from tests.helpers import with_passives
    from uhc_amd import sim as S
    from uhc_amd.model.mjcf import JNT_BALL, ball_variant, hinge_to_ball_qpos
    ball = dataclasses.replace(ball_variant(model), solver=1)
    stiff = with_passives(ball, stiffness=np.where(np.asarray(ball.jnt_type) == JNT_BALL, 30.0, 50.0), qpos_spring=ball.qpos0 + 0.1)
    ctrl = S.make_ctrl(model, action_type="torque", residual_force=False, meta_pd=False, tq_mul=4)
    rng = np.random.default_rng(3)
    n = 2
    q = np.zeros((n, ball.nq))
    for e in range(n):
        qh = standing["qpos"].copy()
        qh[7:] += rng.normal(scale=0.1, size=69)
        qh[2] += 3.0
        q[e] = hinge_to_ball_qpos(model, ball, qh)
    v = rng.normal(scale=0.3, size=(n, ball.nv))
    act = torch.from_numpy(rng.normal(scale=0.1, size=(n, ctrl.action_dim))).cuda()
    tb = torch.zeros(n, 69, dtype=torch.float64, device="cuda")
    out = []
    for m in (ball, stiff):
        b = S.SimBatch(m, ctrl, n)
        b.set_state(torch.from_numpy(q), torch.from_numpy(v))
        b.sync()
        first = b.field(S.F_QACC).cpu().numpy().copy()
        for _ in range(2):
            b.simulate(act, tb)
        b.sync()
        out.append((first, b.field(S.F_QPOS).cpu().numpy().copy(), b.field(S.F_QVEL).cpu().numpy().copy()))
        b.close()
    assert np.abs(out[0][0]).max() > 1.0 and np.isfinite(out[0][1]).all()
    for a, c in zip(*out):
        np.testing.assert_array_equal(a, c)
