"""The Delassus build dispatches on the number of 16-row blocks of a solve, per wave (k_pgs_fast -> delassus_tiles<NB>, NB = 1 .. 4), and accumulates all NB x NB tiles
side by side over the panels.  What an env computes must not depend on where it sits in the batch nor on what its neighbours dispatch to: the twelve states of
tests/delassus_cases.py (row counts on both sides of every block edge, nv = 75: the smallest inputs that reach all four instantiations, with every dense-row placement
tests/test_gpu_delassus.py lists) run in one launch in two orders and must agree BIT FOR BIT, env by env; the same batch run twice must repeat itself bit for bit.
On the general-first path the envs with more than 64 rows go through working sets compacted into the lanes out of row order; those must be order-independent as well
and stay within the existing 1e-5 / 1e-6 of the oracle (tests/test_gpu_delassus.py, the same envs)."""
import dataclasses

import numpy as np
import pytest

from tests.delassus_cases import NEFC_STATES

pytestmark = pytest.mark.gpu

EDGE_COUNTS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
PATHS = (0, 1, 2)  # tier chain from the fast kernel, general tier first, sticky tiers


@pytest.fixture(scope="module")
def selfcol(model):
    from uhc_amd.model.mjcf import self_collision_variant
    from uhc_amd.sim import make_ctrl
    sc = dataclasses.replace(self_collision_variant(model), solver=1)
    return sc, make_ctrl(sc)


@pytest.fixture(scope="module")
def edge_inputs(selfcol):
    """the twelve states and two control steps' actions, one row per state (read-only: the tests index it, none writes to it)"""
    _, ctrl = selfcol
    qpos = np.stack([np.array(NEFC_STATES[k][0]) for k in EDGE_COUNTS])
    qvel = np.stack([np.array(NEFC_STATES[k][1]) for k in EDGE_COUNTS])
    acts = np.random.default_rng(5).normal(scale=0.05, size=(2, len(EDGE_COUNTS), ctrl.action_dim))
    for a in (qpos, qvel, acts):
        a.setflags(write=False)
    return qpos, qvel, acts


def run_from_set_state(b, qpos, qvel, acts):
    """set_state (which runs the forward pass) and one control step per entry of acts; -> F_NEFC of the forward pass, [(F_QACC, F_QPOS, F_QVEL) after each stage]"""
    import torch
    from uhc_amd import sim as S
    b.set_state(torch.from_numpy(qpos.copy()), torch.from_numpy(qvel.copy()))
    b.sync()
    nefc = b.field(S.F_NEFC).cpu().numpy().copy()
    grab = lambda: tuple(b.field(f).cpu().numpy().copy() for f in (S.F_QACC, S.F_QPOS, S.F_QVEL))
    out = [grab()]
    tb = torch.from_numpy(qpos[:, 7:].copy()).cuda()
    for a in acts:
        b.simulate(torch.from_numpy(a.copy()).cuda(), tb)
        b.sync()
        out.append(grab())
    assert int(b.field(S.F_EFC_OVERFLOW).sum().item()) == 0 and int(b.field(S.F_FAIL).sum().item()) == 0
    return nefc, out


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.parametrize("path", PATHS)
def test_mixed_block_counts_in_one_launch_do_not_depend_on_the_order(selfcol, edge_inputs, path):
    """the twelve states and then the same twelve in reverse order in ONE batch: forward pass and two control steps.  Every wave dispatches on its own env's block
    count; an env's qacc, qpos and qvel must be the same bits in both places"""
    from uhc_amd import sim as S
    sc, ctrl = selfcol
    qpos, qvel, acts = edge_inputs
    n = len(EDGE_COUNTS)
    perm = np.concatenate([np.arange(n), np.arange(n)[::-1]])
    b = S.SimBatch(sc, ctrl, 2 * n)
    b.set_kernel_path(path)
    nefc, out = run_from_set_state(b, qpos[perm], qvel[perm], acts[:, perm])
    b.close()
    print("nefc on the device:", nefc.tolist())
    assert nefc.tolist() == [EDGE_COUNTS[i] for i in perm], nefc.tolist()
    for stage, fields in enumerate(out):
        for name, x in zip(("qacc", "qpos", "qvel"), fields):
            fwd, rev = x[:n], x[n:][::-1]  # (undoing the permutation)
            differ = (bits(fwd) != bits(rev)).any(axis=1)
            print(f"path {path} stage {stage} {name}: envs that differ between the two places {np.flatnonzero(differ).tolist()}, max |diff| {np.abs(fwd - rev).max():.3e}")
            assert np.isfinite(x).all()
            assert not differ.any(), (path, stage, name, [EDGE_COUNTS[i] for i in np.flatnonzero(differ)])


@pytest.mark.parametrize("path", PATHS)
def test_the_same_batch_twice_from_set_state_is_bit_equal(selfcol, edge_inputs, path):
    from uhc_amd import sim as S
    sc, ctrl = selfcol
    qpos, qvel, acts = edge_inputs
    b = S.SimBatch(sc, ctrl, len(EDGE_COUNTS))
    b.set_kernel_path(path)
    nefc1, out1 = run_from_set_state(b, qpos, qvel, acts)
    nefc2, out2 = run_from_set_state(b, qpos, qvel, acts)
    b.close()
    assert nefc1.tolist() == list(EDGE_COUNTS) == nefc2.tolist(), (nefc1.tolist(), nefc2.tolist())
    for stage, (f1, f2) in enumerate(zip(out1, out2)):
        for name, x1, x2 in zip(("qacc", "qpos", "qvel"), f1, f2):
            print(f"path {path} stage {stage} {name}: max |run 1 - run 2| {np.abs(x1 - x2).max():.3e}")
            assert (bits(x1) == bits(x2)).all(), (path, stage, name)


def test_working_sets_compacted_out_of_row_order_do_not_depend_on_the_order(selfcol, standing):
    """general tier first: the four envs of test_envs_with_more_than_64_rows_through_the_working_sets (seed 41: 77, 69, 77 and 52 rows), whose working sets are
    compacted into the lanes out of row order, in two batch orders: qacc the same bits, and within 1e-5 / 1e-6 of the oracle"""
    import torch
    from oracle.physics import OracleSim
    from uhc_amd import sim as S
    sc, ctrl = selfcol
    n = 4
    rng = np.random.default_rng(41)
    qpos = np.tile(standing["qpos"], (n, 1))
    qpos[:, 7:] += rng.normal(scale=0.08, size=(n, 69))
    qpos[:, 2] -= 0.004
    qvel = rng.normal(scale=0.3, size=(n, 75))
    got = {}
    for name, order in (("forward", np.arange(n)), ("reverse", np.arange(n)[::-1])):
        b = S.SimBatch(sc, ctrl, n)
        b.set_kernel_path(1)
        b.set_state(torch.from_numpy(qpos[order].copy()), torch.from_numpy(qvel[order].copy()))
        b.sync()
        inv = np.argsort(order)
        got[name] = tuple(b.field(f).cpu().numpy()[inv].copy() for f in (S.F_NEFC, S.F_QACC, S.F_REDO))
        b.close()
    nefc, qacc, redo = got["forward"]
    print("nefc:", nefc.tolist(), "redo:", [hex(int(x)) for x in redo])
    assert nefc.tolist() == [77, 69, 77, 52] == got["reverse"][0].tolist(), (nefc.tolist(), got["reverse"][0].tolist())
    print(f"max |qacc forward - qacc reverse| {np.abs(qacc - got['reverse'][1]).max():.3e}")
    assert (bits(qacc) == bits(got["reverse"][1])).all()
    assert not (redo & S.REDO_SWEPT).all()  # (the exact working-set solve did the work)
    for e in range(n):
        o = OracleSim(sc, ctrl)
        o.desc.solver = 0 if (redo[e] & S.REDO_SWEPT) else 1
        o.set_state(qpos[e], qvel[e])
        assert nefc[e] == o.geti("nefc"), (e, nefc[e], o.geti("nefc"))
        print(f"env {e}: nefc {nefc[e]} max |qacc - oracle| {np.abs(qacc[e] - o.get('qacc')).max():.3e}")
        np.testing.assert_allclose(qacc[e], o.get("qacc"), atol=1e-5, rtol=1e-6)
