"""Friction-loss rows, joint springs and slide joints on the CPU: the oracle against closed forms (so that the checker of tests/test_gpu_passives.py is itself anchored),
`springref` through the model compiler, and the proof that every case of tests/passive_cases.py reaches the branches it is there for -- no case is skipped or filtered on the
GPU side.  The bars of the GPU file are derived and printed here, from the oracle alone."""
import dataclasses

import numpy as np
import pytest

from tests import passive_cases as P
from tests.helpers import cart_model, passive_ctrl, with_passives

G = 9.81
DT = 0.002


def _cart(axis=(0.0, 0.0, 1.0), q=0.0, v=0.0, limit=None, **passives):
    from oracle.physics import OracleSim
    m = with_passives(cart_model(axis, limit), **passives)
    assert m.timestep == DT and abs(m.body_mass[1] - 1.0) < 1e-15
    o = OracleSim(m, passive_ctrl(m))
    o.set_state(np.array([q]), np.array([v]))
    return m, o


def _steps(o, n):
    out = np.zeros((n, 2))
    for t in range(n):
        o.do_simulation(np.zeros(1), np.zeros(1))
        out[t] = o.get("qpos")[0], o.get("qvel")[0]
    return out


# ------------------------------------------------------------------ the oracle against closed forms (both signs of everything: sgn = -1 is the mirrored scene)
@pytest.mark.parametrize("sgn", [1, -1])
def test_friction_loss_below_the_weight_slows_the_fall(sgn):
    """A 1 kg cart at rest on a vertical slide, friction loss 5 N < its weight: the row saturates and the first qacc is -(g - floss / m) along gravity."""
    m, o = _cart(axis=(0, 0, sgn), frictionloss=5.0)
    assert o.geti("nefc") == 1 and o.get("efc_type")[0] == 1
    assert abs(o.get("qacc")[0] - sgn * -(G - 5.0)) < 1e-12, o.get("qacc")
    assert o.get("efc_force")[0] == sgn * 5.0  # saturated at the bound that opposes the fall


@pytest.mark.parametrize("sgn", [1, -1])
def test_friction_loss_above_the_weight_holds_and_the_bound_no_longer_matters(sgn):
    """Friction loss above the weight: the dof is held by a soft row whose impedance at zero violation is d0 = 0.9, so the first qacc is (1 - d0) of the free one --
    whatever the bound, once it no longer binds."""
    acc = []
    for floss in (11.0, 20.0):
        m, o = _cart(axis=(0, 0, sgn), frictionloss=floss)
        assert abs(o.get("efc_force")[0]) < floss
        acc.append(o.get("qacc")[0])
        assert abs(acc[-1] - sgn * -(1 - 0.9) * G) < 1e-12, acc
    assert acc[0] == acc[1]


@pytest.mark.parametrize("sgn", [1, -1])
def test_friction_loss_just_below_the_weight_after_one_second(sgn):
    """Friction loss 9 N against 9.81 N: the cart slides and after 1 s its speed is (g - 9) * 1 s."""
    m, o = _cart(axis=(0, 0, sgn), frictionloss=9.0)
    tr = _steps(o, 500)
    assert abs(tr[-1, 1] - sgn * -(G - 9.0)) < 1e-3, tr[-1]


@pytest.mark.parametrize("sgn", [1, -1])
def test_spring_period_and_amplitude(sgn):
    """A horizontal slide with a spring of 40 N/m and no friction: successive zero crossings are pi / sqrt(k / m) / dt = 248.4 steps apart (within a step), and the amplitude
    after 1000 steps of semi-implicit Euler is the initial displacement."""
    m, o = _cart(axis=(1, 0.3, 0), q=sgn * 0.1, stiffness=40.0)
    assert o.geti("nefc") == 0 and abs(o.get("qacc")[0] - sgn * -4.0) < 1e-13
    tr = _steps(o, 1000)
    cross = np.flatnonzero(np.sign(tr[1:, 0]) != np.sign(tr[:-1, 0]))
    assert len(cross) >= 3 and np.sign(tr[cross[0], 0]) == sgn
    assert (np.abs(np.diff(cross) - np.pi / np.sqrt(40.0) / DT) <= 1.0).all(), np.diff(cross)
    assert abs(np.abs(tr[750:, 0]).max() - 0.1) < 1e-4, np.abs(tr[750:, 0]).max()


@pytest.mark.parametrize("sgn", [1, -1])
def test_slide_rests_on_its_limit(sgn):
    """A vertical slide dropped onto its limit (the lower one; mirrored, the upper one of a slide that points down): one limit row, at rest, and the body where the joint puts it."""
    lim = (-0.2, 0.5) if sgn == 1 else (-0.5, 0.2)
    m, o = _cart(axis=(0, 0, sgn), q=sgn * -0.19, limit=lim)
    assert o.geti("nefc") == 0
    _steps(o, 2500)
    assert o.geti("nefc") == 1 and o.get("efc_type")[0] == 2
    q = o.get("qpos")[0]
    assert abs(o.get("qvel")[0]) < 1e-12 and sgn * q < -0.2 and abs(q) < 0.21, (q, o.get("qvel"))
    assert o.get("efc_force")[0] > 0 and abs(o.get("efc_force")[0] - G) < 1e-6
    assert abs(o.get("xpos")[5] - (m.body_pos[1][2] + sgn * q)) < 1e-15
    np.testing.assert_allclose(o.get("xpos")[3:6], m.body_pos[1] + m.jnt_axis[0] * q, atol=1e-15)


@pytest.mark.parametrize("sgn", [1, -1])
def test_spring_rests_at_qpos_spring_not_at_qpos0(sgn):
    m, o = _cart(axis=(1, 0.3, 0), q=sgn * 0.1, stiffness=40.0, qpos_spring=sgn * 0.1)
    assert m.qpos0[0] == 0.0 and m.qpos_spring[0] == sgn * 0.1
    assert o.get("qacc")[0] == 0.0
    tr = _steps(o, 50)
    assert (tr[:, 0] == sgn * 0.1).all() and (tr[:, 1] == 0.0).all()
    o.set_state(np.zeros(1), np.zeros(1))  # at qpos0 the spring pulls towards qpos_spring
    assert abs(o.get("qacc")[0] - sgn * 4.0) < 1e-13


def test_stiffness_on_ball_and_free_joints_changes_nothing(model, standing):
    """Joint springs act on hinge and slide joints only: a stiffness on the ball joints of the ball-joint humanoid and on its free root leaves every number as it was."""
    from oracle.physics import OracleSim
    from uhc_amd.model.mjcf import JNT_BALL, JNT_FREE, ball_variant, hinge_to_ball_qpos
    from uhc_amd.sim import make_ctrl
    ball = dataclasses.replace(ball_variant(model), solver=1)
    jt = np.asarray(ball.jnt_type)
    assert (jt == JNT_BALL).sum() > 0 and jt[0] == JNT_FREE and set(jt) == {JNT_FREE, JNT_BALL}
    stiff = with_passives(ball, stiffness=np.where(jt == JNT_BALL, 30.0, 50.0), qpos_spring=ball.qpos0 + 0.1)
    assert (stiff.jnt_stiffness > 0).all()
    ctrl = make_ctrl(model, action_type="torque", residual_force=False, meta_pd=False, tq_mul=4)
    rng = np.random.default_rng(3)
    qh = standing["qpos"].copy()
    qh[7:] += rng.normal(scale=0.1, size=69)
    q, v = hinge_to_ball_qpos(model, ball, qh), rng.normal(scale=0.3, size=ball.nv)
    act = rng.normal(scale=0.1, size=ctrl.action_dim)
    out = []
    for m in (ball, stiff):
        o = OracleSim(m, ctrl)
        o.set_state(q, v)
        first = o.get("qacc").copy()
        for _ in range(2):
            o.do_simulation(act, np.zeros(69))
        out.append((first, o.get("qpos").copy(), o.get("qvel").copy()))
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ springref through the model compiler
SPRINGREF_XML = """
<mujoco>
  <compiler angle="{angle}" coordinate="local"/>
  <default><geom contype="0" conaffinity="0"/></default>
  <asset><mesh name="cube" file="unused.stl"/></asset>
  <worldbody>
    <body name="a" pos="0 0 1">
      <inertial pos="0 0 0" mass="1" diaginertia="0.01 0.01 0.01"/>
      <joint name="s" type="slide" axis="1 0 0" stiffness="100" springref="0.1"/>
      <geom type="mesh" mesh="cube"/>
      <body name="b" pos="0 0 -0.2">
        <inertial pos="0 0 -0.1" mass="1" diaginertia="0.01 0.01 0.01"/>
        <joint name="h" type="hinge" axis="0 1 0" stiffness="7" springref="{href}"/>
        <joint name="h2" type="hinge" axis="1 0 0" stiffness="3"/>
        <geom type="mesh" mesh="cube"/>
      </body>
    </body>
  </worldbody>
</mujoco>
"""


def test_compile_mjcf_reads_springref_and_export_mjcf_round_trips_it():
    from tests.helpers import box_triangles
    from uhc_amd.model.mjcf import compile_mjcf, export_mjcf
    meshes = {"cube": box_triangles(0.03, 0.03, 0.03)}
    m = compile_mjcf(SPRINGREF_XML.format(angle="radian", href="-0.25"), meshes=meshes)
    np.testing.assert_array_equal(m.jnt_stiffness, [100.0, 7.0, 3.0])
    np.testing.assert_array_equal(m.qpos_spring, [0.1, -0.25, 0.0])  # (the default is the joint's ref, which this compiler keeps at 0)
    np.testing.assert_array_equal(m.qpos0, [0.0, 0.0, 0.0])
    d = compile_mjcf(SPRINGREF_XML.format(angle="degree", href="-30"), meshes=meshes)
    np.testing.assert_allclose(d.qpos_spring, [0.1, -np.pi / 6, 0.0], rtol=0, atol=1e-16)  # a hinge's springref is an angle, a slide's a length
    xml = export_mjcf(m)
    assert xml.count("springref=") == 3
    back = compile_mjcf(xml)
    np.testing.assert_array_equal(back.qpos_spring, m.qpos_spring)
    np.testing.assert_array_equal(back.jnt_stiffness, m.jnt_stiffness)
    # ... and the spring it describes is the one the oracle applies
    from oracle.physics import OracleSim
    o = OracleSim(m, passive_ctrl(m))
    o.set_state(m.qpos_spring, np.zeros(3))
    g = OracleSim(dataclasses.replace(m, jnt_stiffness=np.zeros(3)), passive_ctrl(m))
    g.set_state(m.qpos_spring, np.zeros(3))
    np.testing.assert_array_equal(o.get("qacc"), g.get("qacc"))  # at its rest position the spring adds nothing


# ------------------------------------------------------------------ zero exclusions: every GPU case reaches what it is there for
def test_case_list_is_the_one_the_gpu_file_names():
    assert tuple(c.name for c in P.cases()) == P.CASE_NAMES
    for c in P.cases():
        assert c.n_env <= 8 and c.steps <= 10 and c.qpos.shape == (c.n_env, c.models[0].nq) and c.act.shape[2] == c.ctrl.action_dim


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_case_reaches_its_branches(name):
    r = P.reference(name)
    c = r["case"]
    limit_rows = 0
    for e, run in enumerate(r["runs"]):
        m = c.model_of(e)
        fdofs = np.flatnonzero(np.asarray(m.dof_frictionloss) > 0)
        assert run["fail"] == 0
        for t, rw in enumerate(run["rows"]):  # the state and the end of every control step
            nf = int((rw["type"] == 1).sum())
            assert nf == len(fdofs), (name, e, t, nf)
            assert (rw["type"][:nf] == 1).all()  # friction-loss rows come first
            np.testing.assert_array_equal(rw["J"][:nf], np.eye(m.nv)[fdofs])
            np.testing.assert_array_equal(rw["floss"][:nf], np.asarray(m.dof_frictionloss)[fdofs])
            assert (np.abs(rw["force"][:nf]) <= rw["floss"][:nf]).all()
            assert P.in_band(c.tier, rw["nefc"], rw["ncon"]), (name, e, t, rw["nefc"], rw["ncon"], c.tier)
            slide = np.asarray(m.jnt_type)[np.asarray(m.dof_jntid)] == 2
            limit_rows += int(((rw["type"] == 2) & (np.abs(rw["J"]) @ slide > 0)).sum())
        # the substeps between two control steps: the sticky maxima bound them from above
        if c.tier != "tier4":
            assert run["max_nefc"] <= dict(fast=P.FAST_ROWS, general=P.GENERAL_ROWS).get(c.tier, P.LARGE_ROWS), (name, e, run["max_nefc"])
            assert run["max_ncon"] <= (P.FAST_CON if c.tier == "fast" else P.GENERAL_CON), (name, e, run["max_ncon"])
    assert (limit_rows > 0) == c.slide_limit, (name, limit_rows)


def _saturation(names):
    hi = lo = inside = 0
    for n in names:
        for run in P.reference(n)["runs"]:
            for rw in run["rows"]:
                fr = rw["type"] == 1
                hi += int((rw["force"][fr] == rw["floss"][fr]).sum())
                lo += int((rw["force"][fr] == -rw["floss"][fr]).sum())
                inside += int((np.abs(rw["force"][fr]) < rw["floss"][fr]).sum())
    return hi, lo, inside


def test_friction_rows_sit_at_both_bounds_and_inside():
    hi, lo, inside = _saturation(P.CASE_NAMES)
    assert hi > 0 and lo > 0 and inside > 0, (hi, lo, inside)
    # the bound's edges do what they are there for: the huge bound never binds (an equality), the tiny one always does (no friction to speak of)
    assert _saturation(["friction_bound_huge"])[:2] == (0, 0) and _saturation(["friction_bound_tiny"])[2] == 0
    # ... and in the tiers behind the fast one too
    for n in ("caterpillar6_solver1", "caterpillar12_solver1", "caterpillar27_solver1", "humanoid_passives"):
        hi, lo, inside = _saturation([n])
        assert hi + lo > 0 and inside > 0, (n, hi, lo, inside)


def test_mirrored_friction_edge_states_mirror_only_the_state():
    for n in ("friction_bound_tiny", "friction_bound_half", "friction_bound_huge"):
        c = P.case(n)
        np.testing.assert_array_equal(c.qpos[1], -c.qpos[0])
        np.testing.assert_array_equal(c.qvel[1], -c.qvel[0])


def test_forward_cases_cover_both_sides_and_the_limit():
    for springs in (False, True):
        r = P.forward_reference(springs)
        c = r["case"]
        q = c.qpos
        lo, hi = c.models[0].jnt_range[0]
        assert c.n_env == 16 and (q[:, 0] < 0).any() and (q[:, 0] > 0).any() and (q[:, 2] < 0).any() and (q[:, 2] > 0).any()
        assert (q[:, 0] < lo).sum() >= 2 and (q[:, 0] > hi).sum() >= 2
        nefc = np.array([run["rows"][0]["nefc"] for run in r["runs"]])
        np.testing.assert_array_equal(nefc > 0, (q[:, 0] < lo) | (q[:, 0] > hi))
        assert springs == bool((np.asarray(c.models[0].qpos_spring) != np.asarray(c.models[0].qpos0)).any())


# ------------------------------------------------------------------ the bars
def test_bars_are_derived_from_the_oracle_and_stay_under_the_cap():
    print("\n" + P.bar_table())
    for n in P.CASE_NAMES:
        r = P.reference(n)
        for k in ("qpos", "qvel"):
            assert P.FACTOR * r["sens"][k] < P.CAP_QPOS_QVEL, (n, k, r["sens"][k])
            assert r["bars"][k] == max(P.FACTOR * r["sens"][k], P.FLOOR[k])
    for springs in (False, True):
        r = P.forward_reference(springs)
        print(r["case"].name, {k: f"{v:.1e}" for k, v in r["bars"].items()})
        for k in ("xpos", "xquat", "xipos", "qM", "qfrc_bias"):
            assert P.FLOOR[k] <= r["bars"][k] < 100 * P.FLOOR[k], (k, r["bars"][k])
