"""The Delassus build on the matrix unit (k_pgs_fast: 16 x 16 tiles of v_mfma_f64_16x16x4_f64, uhc_delassus_tiles.h) against the CPU oracle, on scenes chosen so
that the solve sees the tiles' edges: row counts on both sides of every 16-row block edge (tests/delassus_cases.py: the self-colliding humanoid, nv = 75 -- a padded
last panel -- with packed rows and dense body-body rows in one solve), envs with more than 64 rows (the general tier compacts its working sets into the lanes out of
row order), a windowed island, and friction-loss rows (the sweeps on the same A).  Dense rows where the gather can go wrong -- alone in a row block of their own
beside the packed rows they couple to, several coupling to each other, in lane 0, in the last valid lane -- are asserted from the oracle's row list (row_layout).
The sizes: nv = 75, nv = 99 (the ball-joint humanoid among boxes: rows whose dofs lie in the second word of the chain masks only, and a dense row across both),
nv = 32 (caterpillar_model: rows of the longest chain the kernels take), nv = 1 (a pendulum at its limit).  Every kernel path: the tier chain from the fast kernel,
general-only, sticky tiers.  Tolerances: those of the existing tests for the same comparisons -- forward qacc of the humanoid atol 1e-5 / rtol 1e-6 and trajectories 1e-5
on qpos (test_gpu_selfcollision), the free boxes 1e-6 / 1e-6 (the same file), the caterpillar 1e-7 (1 + max |qacc|) (the same file), one control step from the device's
state 1e-10 / 1e-8 (its raft of boxes), an exact solve on both sides 1e-8 / 1e-9 (tests/passive_cases.py)."""
import dataclasses

import numpy as np
import pytest

from tests.delassus_cases import NEFC_STATES

pytestmark = pytest.mark.gpu

EDGE_COUNTS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
PATHS = {"fast": 0, "general": 1, "sticky": 2}


def row_layout(o, m):
    """The rows of the oracle's last forward pass, one letter each, in row order (the device enumerates them in the same order: lane = row in the fast kernel):
    'p' a row along one dof chain (friction loss, limit, a contact with the floor or a fixed body), 'D' a contact row between two moving bodies (a dense row)."""
    t, g1, g2 = (o.get(k).astype(int) for k in ("efc_type", "con_geom1", "con_geom2"))
    gb = np.asarray(m.geom_bodyid)
    out, c, r = "", 0, 0
    while r < len(t):
        if t[r] < 3:
            out, r = out + "p", r + 1
            continue
        k = 1 if t[r] == 3 else 4
        out += ("D" if gb[g1[c]] != 0 and gb[g2[c]] != 0 else "p") * k
        r, c = r + k, c + 1
    return out


@pytest.fixture(scope="module")
def selfcol(model):
    from uhc_amd.model.mjcf import self_collision_variant
    from uhc_amd.sim import make_ctrl
    sc = dataclasses.replace(self_collision_variant(model), solver=1)
    return sc, make_ctrl(sc)


@pytest.fixture(scope="module")
def edge_reference(selfcol):
    """the oracle's forward pass of every edge state, computed once: (nefc, ncon, qacc)"""
    from oracle.physics import OracleSim
    sc, ctrl = selfcol
    ref = {}
    for k in EDGE_COUNTS:
        o = OracleSim(sc, ctrl)
        o.set_state(np.array(NEFC_STATES[k][0]), np.array(NEFC_STATES[k][1]))
        ref[k] = (o.geti("nefc"), o.geti("ncon"), o.get("qacc").copy())
        ref[k, "rows"] = row_layout(o, sc)
    return ref


def test_edge_states_place_dense_rows_at_the_gathers_edges(edge_reference):
    """what the states of delassus_cases.py put where (no device needed for this, but the device cases below rest on it): a single dense row in lane 0 which is also the
    last lane; dense rows alone in row block 2 resp. 3, in the last valid lane, coupling to packed rows of the blocks below; twelve dense rows -- the fast layout's
    capacity -- coupling to each other behind 20 packed rows; states without any packed row; a state without any dense row"""
    rows = {k: edge_reference[k, "rows"] for k in EDGE_COUNTS}
    assert all(len(rows[k]) == k for k in EDGE_COUNTS)
    assert rows[1] == "D"
    assert rows[33] == "p" * 32 + "D" and rows[49] == "p" * 48 + "D"
    assert rows[32] == "p" * 20 + "D" * 12
    assert rows[47] == "p" * 40 + "D" * 7 and rows[48] == "p" * 40 + "D" * 8
    assert all(rows[k] == "D" * k for k in (15, 16, 17)) and rows[64] == "p" * 64


@pytest.mark.parametrize("path", sorted(PATHS))
def test_row_counts_on_both_sides_of_every_tile_edge(selfcol, edge_reference, path):
    """forward pass and two control steps of the twelve states in one batch; each listed count must be REACHED on the device (F_NEFC), not merely aimed at"""
    import torch
    from oracle.physics import OracleSim
    from uhc_amd import sim as S
    sc, ctrl = selfcol
    n = len(EDGE_COUNTS)
    qpos = np.stack([np.array(NEFC_STATES[k][0]) for k in EDGE_COUNTS])
    qvel = np.stack([np.array(NEFC_STATES[k][1]) for k in EDGE_COUNTS])
    b = S.SimBatch(sc, ctrl, n)
    b.set_kernel_path(PATHS[path])
    b.set_state(torch.from_numpy(qpos), torch.from_numpy(qvel))
    b.sync()
    ncon, nefc, qacc, redo = (b.field(f).cpu().numpy() for f in (S.F_NCON, S.F_NEFC, S.F_QACC, S.F_REDO))
    print("nefc on the device:", nefc.tolist(), "redo:", [hex(int(x)) for x in redo])
    assert nefc.tolist() == list(EDGE_COUNTS), nefc.tolist()
    assert not (redo & S.REDO_SWEPT).any() and not (redo & S.REDO_DROPPED).any(), [hex(int(x)) for x in redo]
    if path == "fast":  # the states with at most 12 dense rows are the fast kernel's own: lane = row there, so the dense rows sit in the lanes row_layout names
        assert all(redo[EDGE_COUNTS.index(k)] == 0 for k in (1, 32, 33, 47, 48, 49)), redo.tolist()
    elif path == "general":
        assert (redo & S.REDO_GENERAL).all()
    for e, k in enumerate(EDGE_COUNTS):
        r_nefc, r_ncon, r_qacc = edge_reference[k]
        assert r_nefc == k and NEFC_STATES[k][2] == r_ncon == ncon[e], (k, r_nefc, r_ncon, ncon[e])
        np.testing.assert_allclose(qacc[e], r_qacc, atol=1e-5, rtol=1e-6, err_msg=f"nefc {k}")
    os_ = [OracleSim(sc, ctrl) for _ in range(n)]
    for e in range(n):
        os_[e].set_state(qpos[e], qvel[e])
    rng = np.random.default_rng(5)
    tb = torch.from_numpy(qpos[:, 7:].copy()).cuda()
    worst = 0.0
    for t in range(2):
        act = rng.normal(scale=0.05, size=(n, ctrl.action_dim))
        b.simulate(torch.from_numpy(act).cuda(), tb)
        b.sync()
        gq = b.field(S.F_QPOS).cpu().numpy()
        redo = b.field(S.F_REDO).cpu().numpy()
        for e in range(n):
            os_[e].do_simulation(act[e], qpos[e, 7:], redo=redo[e])
            worst = max(worst, np.abs(gq[e] - os_[e].get("qpos")).max())
    print("worst |qpos - oracle| over two control steps:", worst)
    assert worst < 1e-5, worst
    assert int(b.field(S.F_EFC_OVERFLOW).sum().item()) == 0 and int(b.field(S.F_FAIL).sum().item()) == 0
    b.close()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_envs_with_more_than_64_rows_through_the_working_sets(selfcol, standing, path):
    """standing on the floor with body-body contacts: more than 64 rows per env, solved by working sets of <= 64 rows compacted into the lanes (dense rows land
    in whatever lane the compaction gives them)"""
    import torch
    from oracle.physics import OracleSim
    from uhc_amd import sim as S
    sc, ctrl = selfcol
    n = 4
    rng = np.random.default_rng(41)  # (chosen on the CPU with the oracle: 77, 69, 77 and 52 rows)
    qpos = np.tile(standing["qpos"], (n, 1))
    qpos[:, 7:] += rng.normal(scale=0.08, size=(n, 69))
    qpos[:, 2] -= 0.004
    qvel = rng.normal(scale=0.3, size=(n, 75))
    b = S.SimBatch(sc, ctrl, n)
    b.set_kernel_path(PATHS[path])
    b.set_state(torch.from_numpy(qpos), torch.from_numpy(qvel))
    b.sync()
    nefc, qacc, redo = (b.field(f).cpu().numpy() for f in (S.F_NEFC, S.F_QACC, S.F_REDO))
    print("nefc:", nefc.tolist(), "redo:", [hex(int(x)) for x in redo])
    assert (nefc > 64).sum() >= 2, nefc.tolist()
    for e in range(n):
        o = OracleSim(sc, ctrl)
        o.desc.solver = 0 if (redo[e] & S.REDO_SWEPT) else 1
        o.set_state(qpos[e], qvel[e])
        assert nefc[e] == o.geti("nefc"), (e, nefc[e], o.geti("nefc"))
        np.testing.assert_allclose(qacc[e], o.get("qacc"), atol=1e-5, rtol=1e-6)
    assert not (redo & S.REDO_SWEPT).all()  # (the exact working-set solve did the work)
    b.close()


def test_friction_loss_rows_sweep_the_same_matrix(model, standing):
    """friction loss on 40 hinge dofs of the floor-only humanoid: box-constrained rows, so the solve takes the sweeps on the A of the same build -- one env airborne (the 40
    loss rows alone, in the fast kernel), two on the floor (loss rows + contact rows: more than 64, the general tier's sweeps).  The bar is the one of
    tests/passive_cases.py where both sides sweep to the model's tolerance: 1e-5 + 1e-6 |qacc|."""
    import torch
    from oracle.physics import OracleSim
    from tests.helpers import with_passives
    from uhc_amd import sim as S
    from uhc_amd.sim import make_ctrl
    loss = np.zeros(model.nv)
    loss[6:46] = 0.3
    m = dataclasses.replace(with_passives(model, frictionloss=loss), solver=1)
    ctrl = make_ctrl(m)
    n = 3
    rng = np.random.default_rng(8)
    qpos = np.tile(standing["qpos"], (n, 1))
    qpos[:, 7:] += rng.normal(scale=0.05, size=(n, 69))
    qpos[:, 2] += np.array([1.0, 0.0, 0.002])
    qvel = rng.normal(scale=0.3, size=(n, 75))
    b = S.SimBatch(m, ctrl, n)
    b.set_state(torch.from_numpy(qpos), torch.from_numpy(qvel))
    b.sync()
    nefc, qacc = (b.field(f).cpu().numpy() for f in (S.F_NEFC, S.F_QACC))
    print("nefc:", nefc.tolist())
    assert 40 <= nefc[0] <= 64 and (nefc[1:] > 64).all(), nefc.tolist()  # (40 loss rows, + a joint limit or two; the others beyond the fast kernel)
    for e in range(n):
        o = OracleSim(m, ctrl)
        o.desc.solver = 0  # friction-loss rows: the sweeps, on the device and in the oracle
        o.set_state(qpos[e], qvel[e])
        assert nefc[e] == o.geti("nefc")
        print(f"env {e}: nefc {nefc[e]} max |qacc - oracle| {np.abs(qacc[e] - o.get('qacc')).max():.3e}")
        np.testing.assert_allclose(qacc[e], o.get("qacc"), atol=1e-5, rtol=1e-6)
    b.close()


@pytest.mark.parametrize("path", ["fast", "general"])
def test_two_boxes_a_dense_row_alone_in_the_next_row_block(path):
    """two free boxes (nv = 12).  Stacked: 16 pyramid rows of the lower box on the floor fill row block 0, the box-box row is row 16 -- alone in block 1, the last
    valid lane, coupling to every packed row of block 0 through the lower box's dofs.  Touching in the air: the dense row is the only row, lane 0."""
    import torch
    from oracle.physics import OracleSim
    from tests.helpers import passive_ctrl, two_box_model
    from uhc_amd import sim as S
    m = dataclasses.replace(two_box_model(0.1, 0.06), solver=1)
    q = np.array([[0, 0, 0.0998, 1, 0, 0, 0, 0.01, -0.02, 0.2 + 0.0598, 1, 0, 0, 0.0],
                  [0, 0, 0.0998, 1, 0, 0, 0, 0.05, 0.03, 0.2 + 0.07, 0.9689, 0.2474, 0, 0.0],
                  [0, 0, 2.0, 1, 0, 0, 0, 0.01, -0.02, 2.1 + 0.0598, 1, 0, 0, 0.0]])
    v = np.random.default_rng(2).normal(scale=0.2, size=(3, 12))
    b = S.SimBatch(m, passive_ctrl(m), 3)
    b.set_kernel_path(PATHS[path])
    b.set_state(torch.from_numpy(q), torch.from_numpy(v))
    b.sync()
    nefc, qacc, redo = (b.field(f).cpu().numpy() for f in (S.F_NEFC, S.F_QACC, S.F_REDO))
    want = ["p" * 16 + "D", "p" * 16 + "D", "D"]
    for e in range(3):
        o = OracleSim(m)
        o.set_state(q[e], v[e])
        assert row_layout(o, m) == want[e] and nefc[e] == len(want[e]), (e, row_layout(o, m), nefc[e])
        print(f"boxes env {e}: rows {want[e]} max |qacc - oracle| {np.abs(qacc[e] - o.get('qacc')).max():.3e}")
        np.testing.assert_allclose(qacc[e], o.get("qacc"), atol=1e-6, rtol=1e-6)
    assert not (redo & S.REDO_SWEPT).any() and (path != "fast" or (redo == 0).all()), redo.tolist()
    b.close()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_nv_99_rows_in_the_second_word_of_the_chain_masks(path):
    """the ball-joint humanoid among four boxes (nv = 99, configs[4]'s class), the humanoid in the air: 16 rows of a box on the floor, whose chains are dofs 75 .. 80 --
    the second 64-bit word of the masks alone, the walk's restart at dof 64 --, a self-contact of the humanoid (a dense row over all dofs) and the row of a box
    standing on that box (dense, its entries at dofs 75 .. 86)."""
    import torch
    from oracle.physics import OracleSim
    from tests.test_batch_plan_cpu import model_class
    from uhc_amd import sim as S
    m, ctrl = model_class("ball_boxes")
    assert m.nv == 99 and m.nq == 127 and list(np.asarray(m.body_dofadr)[-4:]) == [75, 81, 87, 93]
    n = 2
    q = np.tile(m.qpos0, (n, 1))
    q[:, 2] += 5.0
    q[:, 99 + 2] = 0.1495
    q[:, 99 + 7:99 + 10] = q[:, 99:99 + 3] + np.array([0.02, -0.01, 0.2995])
    q[:, 99 + 14 + 2], q[:, 99 + 21 + 2] = 3.0, 4.0
    q[1, 99 + 7] += 0.03
    v = np.random.default_rng(6).normal(scale=0.1, size=(n, 99))
    b = S.SimBatch(m, ctrl, n)
    b.set_kernel_path(PATHS[path])
    b.set_state(torch.from_numpy(q), torch.from_numpy(v))
    b.sync()
    nefc, qacc, redo = (b.field(f).cpu().numpy() for f in (S.F_NEFC, S.F_QACC, S.F_REDO))
    for e in range(n):
        o = OracleSim(m, ctrl)
        o.set_state(q[e], v[e])
        rows = row_layout(o, m)
        assert rows == "p" * 16 + "DD" and nefc[e] == 18, (rows, nefc[e])
        print(f"nv 99 env {e}: rows {rows} redo {hex(int(redo[e]))} max |qacc - oracle| {np.abs(qacc[e] - o.get('qacc')).max():.3e}")
        np.testing.assert_allclose(qacc[e], o.get("qacc"), atol=1e-5, rtol=1e-6)
    assert not (redo & S.REDO_SWEPT).any() and (path != "fast" or (redo == 0).all()), redo.tolist()
    b.close()


@pytest.mark.parametrize("path", ["fast", "general"])
def test_rows_of_the_longest_chain(path):
    """caterpillar_model: 27 boxes on one chain of 32 dofs, as long as the kernels' row registers (UHC_YM).  Pitched nose-up with the last hinge bent back, the animal
    stands on its LAST box alone: 16 pyramid rows, every one along the full chain."""
    import torch
    from oracle.physics import OracleSim
    from scipy.spatial.transform import Rotation as sR
    from tests.helpers import caterpillar_model, passive_ctrl
    from uhc_amd import sim as S
    m = dataclasses.replace(caterpillar_model(27), solver=1)
    ctrl = passive_ctrl(m)
    assert m.nv == 32
    q = m.qpos0.copy()
    q[7:] = 0.0
    q[3:7] = np.roll(sR.from_rotvec([0, 0.5, 0]).as_quat(), 1)
    q[7 + 25] = -0.5
    q[2] = 2.79
    v = np.random.default_rng(9).normal(scale=0.05, size=32)
    b = S.SimBatch(m, ctrl, 1)
    b.set_kernel_path(PATHS[path])
    b.set_state(torch.from_numpy(q[None]), torch.from_numpy(v[None]))
    b.sync()
    o = OracleSim(m, ctrl)
    o.set_state(q, v)
    last_geom = int(np.flatnonzero(np.asarray(m.geom_bodyid) == m.nbody - 1)[0])
    assert o.geti("nefc") == 16 and set(o.get("con_geom2").astype(int)) == {last_geom}, (o.geti("nefc"), o.get("con_geom2"))
    assert int(b.field(S.F_NEFC)[0].item()) == 16
    ga, oa = b.field(S.F_QACC)[0].cpu().numpy(), o.get("qacc")
    print(f"chain of 32: max |qacc - oracle| {np.abs(ga - oa).max():.3e} of max |qacc| {np.abs(oa).max():.3e}")
    np.testing.assert_allclose(ga, oa, atol=1e-7 * (1 + np.abs(oa).max()), rtol=0)
    redo = int(b.field(S.F_REDO)[0].item())
    assert not redo & S.REDO_SWEPT and (path != "fast" or redo == 0), hex(redo)
    b.close()


def test_one_dof_one_row():
    """a pendulum past the upper end of its range: nv = 1 (one panel, three of its four dofs padding), one limit row"""
    import torch
    from oracle.physics import OracleSim
    from tests.helpers import passive_ctrl, pendulum_model
    from uhc_amd import sim as S
    m = dataclasses.replace(pendulum_model(), jnt_limited=np.array([1], dtype=np.int32), jnt_range=np.array([[-0.3, 0.3]]), solver=1)
    q, v = np.array([[0.31], [-0.305]]), np.array([[0.5], [-0.2]])
    b = S.SimBatch(m, passive_ctrl(m), 2)
    b.set_state(torch.from_numpy(q), torch.from_numpy(v))
    b.sync()
    for e in range(2):
        o = OracleSim(m)
        o.set_state(q[e], v[e])
        assert o.geti("nefc") == 1 and int(b.field(S.F_NEFC)[e].item()) == 1
        np.testing.assert_allclose(b.field(S.F_QACC)[e].cpu().numpy(), o.get("qacc"), atol=1e-8, rtol=1e-9)
    assert int(b.field(S.F_REDO).sum().item()) == 0
    b.close()


def test_windowed_island_of_more_than_64_force_rows(model, standing, monkeypatch):
    """the raft of test_island_with_more_than_64_force_rows_is_solved_exactly at its smallest: one env, two control steps, three tiers (UHC_TIERS=3), so that the island
    of seven boxes goes through WINDOWS of 64 rows -- working sets whose right-hand side carries the rows outside -- each built by the same k_pgs_fast"""
    import torch
    from oracle.physics import OracleSim
    from uhc_amd import sim as S
    from uhc_amd.model.mjcf import add_free_bodies, self_collision_variant
    from uhc_amd.model.shapes import box_triangles
    from uhc_amd.sim import make_ctrl
    monkeypatch.setenv("UHC_TIERS", "3")
    K = 7
    yaw = [0.06 * (-1) ** k for k in range(K)]
    poses = np.array([[1.0 + 0.305 * k, 1.0 + 0.01 * k, 0.1495, np.cos(y / 2), 0, 0, np.sin(y / 2)] for k, y in enumerate(yaw)], dtype=np.float64)
    m = add_free_bodies(self_collision_variant(model), [box_triangles(0.15, 0.15, 0.15)] * K, poses, density=5.0 / 0.027)
    m = dataclasses.replace(m, solver=1)
    ctrl = make_ctrl(model, action_type="torque", residual_force=False, meta_pd=False, tq_mul=4)
    q = m.qpos0.copy()[None]
    q[0, :76] = standing["qpos"]
    b = S.SimBatch(m, ctrl, 1)
    b.set_state(torch.from_numpy(q), torch.zeros(1, m.nv, dtype=torch.float64))
    b.sync()
    o = OracleSim(m, ctrl)
    tb = torch.zeros(1, 69, dtype=torch.float64, device="cuda")
    act = np.zeros((1, ctrl.action_dim))
    windowed, worst_q, worst_v = 0, 0.0, 0.0
    for t in range(2):
        gq0, gv0 = b.field(S.F_QPOS).cpu().numpy().copy(), b.field(S.F_QVEL).cpu().numpy().copy()
        b.simulate(torch.from_numpy(act).cuda(), tb)
        b.sync()
        redo = int(b.field(S.F_REDO)[0].item())
        windowed += int((redo & S.REDO_WINDOWED) != 0)
        assert not redo & S.REDO_SWEPT and not redo & S.REDO_PRIMAL, hex(redo)
        o.set_state(gq0[0], gv0[0])
        o.do_simulation(act[0], np.zeros(69))
        worst_q = max(worst_q, np.abs(b.field(S.F_QPOS)[0].cpu().numpy() - o.get("qpos")).max())
        worst_v = max(worst_v, np.abs(b.field(S.F_QVEL)[0].cpu().numpy() - o.get("qvel")).max())
    print(f"windowed env-steps {windowed} / 2, max nefc {o.geti('max_nefc')}; one control step from the device's state: |dqpos| {worst_q:.2e} |dqvel| {worst_v:.2e}")
    assert windowed > 0, "no island exceeded 64 force-carrying rows: the scene no longer exercises the windows"
    assert worst_q < 1e-10 and worst_v < 1e-8, (worst_q, worst_v)
    b.close()
