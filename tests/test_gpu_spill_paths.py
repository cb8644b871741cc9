"""The step kernels after their spilled values moved (loop invariants recomputed at their use instead of reloaded from scratch, the model blob addressed from a
scalar base): device against the oracle on the paths where a value that now lives somewhere else would show -- a batch with one model blob per env, a chunk
boundary and a hand-on in mid-step, the edges of the fast tier's register-resident solve (no rows, exactly 64 rows, every body-body slot taken), and the same step
twice from the same state.

Every comparison is of ONE control step from a state both sides were just given (set_state on the device and on the oracle: `resynced`), so the dynamics do not
amplify anything: 1e-9 on qpos, qvel and qacc, and on the stored qM where the test names it.  Every kernel path (uhc_batch_set_kernel_path 0: fast tier then the
chained general tier, 1: general tier alone, 2: sticky tiers with their queue consumers), 4 envs.  (Largest differences met over all cases: qpos 1.4e-15, qvel
3.8e-14, qacc 2.0e-11, qM 1.4e-14.)

The states of the edge cases come from the oracle's own trajectories of this repository's models (tests/golden/spill_paths_states.npz: q64 / v64 -- the floor-only
asset model on both feet, 16 contacts x 4 pyramid rows = 64 rows; qtwo2 / vtwo2 -- the self-colliding variant with 2 body-body contacts among 14, 50 rows)."""
import contextlib
import dataclasses
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = (0, 1, 2)
TOL = 1e-9


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def edge_states():
    z = np.load(os.path.join(ROOT, "tests", "golden", "spill_paths_states.npz"))
    return {k: z[k] for k in z.files}


def _batch(models, ctrl, n, path, env_model=None, **env):
    from uhc_amd.sim import SimBatch
    with _env(UHC_FORCE_GENERAL=0, **env):
        b = SimBatch(models, ctrl, n, env_model=env_model) if env_model is not None else SimBatch(models, ctrl, n)
    b.set_kernel_path(path)
    return b


def _resynced_steps(b, oracles, qpos, qvel, acts, tb, where, check_qm=False):
    """len(acts) control steps, each from the device's own state of the step before, handed to BOTH sides by set_state.  Returns the per-step (why, redo, nefc after
    set_state) words of the device."""
    import torch
    from uhc_amd import sim as S
    n = qpos.shape[0]
    q, v = qpos.copy(), qvel.copy()
    tbd = torch.from_numpy(tb).cuda()
    words = []
    for t, act in enumerate(acts):
        b.set_state(torch.from_numpy(q), torch.from_numpy(v))
        b.sync()
        nefc0 = b.field(S.F_NEFC).cpu().numpy().copy()
        for e in range(n):
            oracles[e].set_state(q[e], v[e])
        b.simulate(torch.from_numpy(act).cuda(), tbd)
        b.sync()
        redo = b.field(S.F_REDO).cpu().numpy()
        gq, gv, ga, gm = (b.field(f).cpu().numpy() for f in (S.F_QPOS, S.F_QVEL, S.F_QACC, S.F_QM))
        assert int(b.field(S.F_FAIL).sum().item()) == 0, f"{where} step {t}: a bad-value flag"
        for e in range(n):
            o = oracles[e]
            o.do_simulation(act[e], tb[e], redo=redo[e])
            dq, dv, da = (np.abs(x - o.get(k)).max() for x, k in ((gq[e], "qpos"), (gv[e], "qvel"), (ga[e], "qacc")))
            dm = np.abs(gm[e] - o.get("qM")).max()
            print(f"{where} step {t} env {e}: |dqpos| {dq:.2e} |dqvel| {dv:.2e} |dqacc| {da:.2e} |dqM| {dm:.2e}  rows {o.geti('nefc')} redo {int(redo[e]):#x}")
            assert dq < TOL and dv < TOL and da < TOL, f"{where} step {t} env {e}: qpos {dq:.2e} qvel {dv:.2e} qacc {da:.2e}"
            if check_qm:
                assert dm < TOL, f"{where} step {t} env {e}: stored qM {dm:.2e}"
        words.append((b.field(S.F_HANDON_WHY).cpu().numpy().copy(), redo.copy(), nefc0))
        q, v = gq.copy(), gv.copy()
    assert b.give_ups() == 0
    return words


def _assert_fast_tier_served(words, envs, path, where):
    """The fast tier ran at least the first substep of these envs' step -- the state the test hands over is the edge, so k_pgs_fast solved AT the edge: either the
    fast tier finished the step (REDO_GENERAL clear) or it handed the env on in a later substep.  (Path 1 has no fast tier.)"""
    from uhc_amd.sim import REDO_GENERAL, WHY_FAST_SHIFT, WHY_FIELD, WHY_SUBSTEP_SHIFT
    if path == 1:
        return
    why, redo, _ = words
    for e in envs:
        whole = (int(redo[e]) & REDO_GENERAL) == 0
        later = ((int(why[e]) >> WHY_FAST_SHIFT) & WHY_FIELD) != 0 and ((int(why[e]) >> WHY_SUBSTEP_SHIFT) & WHY_FIELD) >= 1
        assert whole or later, f"{where} env {e}: the fast tier never solved this env's first substep (redo {int(redo[e]):#x}, why {int(why[e]):#x})"


@pytest.mark.parametrize("path", PATHS)
def test_two_scaled_models_in_one_batch(model, ctrl, standing, path):
    """One blob per env (as bench.py --shapes builds them: every body its own length scale): a stage that read its constants from the wrong blob would compute
    another body.  2 control steps."""
    from oracle.physics import OracleSim
    from uhc_amd import sim as S
    from uhc_amd.model.mjcf import kinematics_np, quat_to_mat, scale_model_per_body
    rng = np.random.default_rng(7)
    models = [scale_model_per_body(model, np.r_[1.0, rng.uniform(0.85, 1.15, size=model.nbody - 1)]) for _ in range(2)]

    def lowest(m, q):
        xp, xq, _, _ = kinematics_np(m, q)
        return min((m.mesh_vert[m.geom_vertadr[g]:m.geom_vertadr[g] + m.geom_vertnum[g]] @ quat_to_mat(xq[m.geom_bodyid[g]]).T + xp[m.geom_bodyid[g]])[:, 2].min()
                   for g in range(m.ngeom) if m.geom_type[g] == 7)

    env_model = [0, 1, 1, 0]
    n = len(env_model)
    r2 = np.random.default_rng(11)
    qpos = np.tile(standing["qpos"], (n, 1))
    qpos[:, 7:] += r2.normal(scale=0.03, size=(n, model.nu))
    qvel = r2.normal(scale=0.1, size=(n, model.nv))
    for e in range(n):  # the feet where the stock model has them: rows from the first substep on
        qpos[e, 2] += lowest(model, qpos[e]) - lowest(models[env_model[e]], qpos[e])
    acts = [r2.normal(scale=0.1, size=(n, ctrl.action_dim)) for _ in range(2)]
    b = _batch(models, ctrl, n, path, env_model=env_model)
    oracles = [OracleSim(models[env_model[e]], ctrl) for e in range(n)]
    _resynced_steps(b, oracles, qpos, qvel, acts, qpos[:, 7:].copy(), f"two models, path {path}", check_qm=True)
    gm = b.field(S.F_QM).cpu().numpy()
    assert np.abs(gm[0] - gm[1]).max() > 1e-3, "the two models are the same body"
    assert sum(o.geti("ncon") for o in oracles) > 0, "nobody touches the floor"


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("chunk", (1, 5))
def test_chunk_boundary_and_hand_on_in_mid_step(model, standing, chunk, path):
    """The drop scene of tests/test_gpu_fast_chunks.py (self-colliding humanoids a few centimetres above the floor, no action): in the third control step the impact
    takes the rows from <= 35 past 64 around substep 10, so the fast tier hands the env on in mid-step, behind one or more chunk boundaries.  M parked across the
    substeps and the constants the stages recompute survive both; the qM the step stores is the oracle's."""
    from oracle.physics import OracleSim
    from uhc_amd.model.mjcf import self_collision_variant
    from uhc_amd.sim import REDO_GENERAL, WHY_FAST_SHIFT, WHY_FIELD, WHY_SUBSTEP_SHIFT, make_ctrl
    sc = dataclasses.replace(self_collision_variant(model), solver=1)
    c = make_ctrl(sc)
    n = 4
    rng = np.random.default_rng(67)
    qpos = np.tile(standing["qpos"], (n, 1))
    qpos[:, 7:] += rng.normal(scale=0.002, size=(n, 69))
    qpos[:, 2] += np.array([0.0367, 0.04, 0.0433, 0.0467])
    qvel = np.zeros((n, sc.nv))
    acts = [np.zeros((n, c.action_dim)) for _ in range(4)]
    b = _batch(sc, c, n, path, UHC_FAST_CHUNK=chunk)
    oracles = [OracleSim(sc, c) for _ in range(n)]
    words = _resynced_steps(b, oracles, qpos, qvel, acts, qpos[:, 7:].copy(), f"drop, chunk {chunk}, path {path}", check_qm=True)
    if path != 1:  # (path 1 has no fast tier to hand anything on)
        mid = sum(int((((redo & REDO_GENERAL) != 0) & (((why >> WHY_FAST_SHIFT) & WHY_FIELD) != 0) & (((why >> WHY_SUBSTEP_SHIFT) & WHY_FIELD) >= 1)).sum()) for why, redo, _ in words)
        assert mid >= 1, "no env was handed on in mid-step"


@pytest.mark.parametrize("path", PATHS)
def test_no_rows_beside_exactly_64_rows(model, standing, edge_states, path):
    """The floor-only asset model: airborne envs (nefc == 0: the solve is skipped altogether) beside envs at exactly 64 rows and 16 contacts, the fast tier's caps --
    every lane of the register-resident solve owns a row, the last column chunk is full."""
    from oracle.physics import OracleSim
    from uhc_amd import sim as S
    from uhc_amd.sim import make_ctrl
    m = dataclasses.replace(model, solver=1)
    c = make_ctrl(m)
    n = 4
    qpos = np.tile(standing["qpos"], (n, 1))
    qvel = np.zeros((n, m.nv))
    qpos[[0, 2], 2] += 50.0
    qvel[[0, 2]] = np.random.default_rng(3).normal(scale=0.3, size=(2, m.nv))
    qpos[[1, 3]], qvel[[1, 3]] = edge_states["q64"], edge_states["v64"]
    qvel[3] *= 1.0 + 1e-6  # (not the same env twice)
    acts = [np.zeros((n, c.action_dim))]
    b = _batch(m, c, n, path)
    oracles = [OracleSim(m, c) for _ in range(n)]
    words = _resynced_steps(b, oracles, qpos, qvel, acts, edge_states["q64"][7:][None].repeat(n, 0).copy(), f"0 / 64 rows, path {path}")
    assert words[0][2].tolist() == [0, 64, 0, 64], words[0][2]
    _assert_fast_tier_served(words[0], (1, 3), path, f"0 / 64 rows, path {path}")
    assert int(b.field(S.F_NEFC).cpu().numpy()[0]) == 0


@pytest.mark.parametrize("path", PATHS)
def test_body_body_rows_in_every_dense_slot(model, standing, edge_states, path):
    """The self-colliding variant with the fast tier planned for TWO body-body rows (UHC_FAST_DENSE=52,2): envs with exactly 2 body-body contacts among 14 (50 rows)
    fill every dense slot -- the Delassus columns of the dense rows, their AGPR park and the scatter of their forces all run at their capacity -- beside envs whose
    7 body-body contacts (the standing pose in the air) do not fit the two slots and go to the general tier at once."""
    from oracle.physics import OracleSim
    from uhc_amd.model.mjcf import self_collision_variant
    from uhc_amd.sim import make_ctrl
    sc = dataclasses.replace(self_collision_variant(model), solver=1)
    c = make_ctrl(sc)
    n = 4
    qpos = np.tile(standing["qpos"], (n, 1))
    qvel = np.zeros((n, sc.nv))
    qpos[[1, 3], 2] += 50.0
    qpos[[0, 2]], qvel[[0, 2]] = edge_states["qtwo2"], edge_states["vtwo2"]
    qvel[2] *= 1.0 + 1e-6
    acts = [np.zeros((n, c.action_dim))]
    b = _batch(sc, c, n, path, UHC_FAST_DENSE="52,2")
    oracles = [OracleSim(sc, c) for _ in range(n)]
    words = _resynced_steps(b, oracles, qpos, qvel, acts, edge_states["qtwo2"][7:][None].repeat(n, 0).copy(), f"dense slots, path {path}")
    assert words[0][2][[0, 2]].tolist() == [50, 50], words[0][2]
    _assert_fast_tier_served(words[0], (0, 2), path, f"dense slots, path {path}")
    gb = np.asarray(sc.geom_bodyid)
    for e in (0, 2):  # the scene is what it says: 2 contacts between moving bodies at the state handed over
        t = OracleSim(sc, c)
        t.set_state(qpos[e], qvel[e])
        g1, g2 = t.get("con_geom1").astype(int), t.get("con_geom2").astype(int)
        assert int(((gb[g1] > 0) & (gb[g2] > 0)).sum()) == 2


@pytest.mark.parametrize("path", PATHS)
def test_the_same_step_twice_gives_the_same_bits(model, standing, edge_states, path):
    """A stage that reloads something the step itself overwrites (a table entry, a parked value) would compute the second step from other inputs than the first:
    the drop scene through its impact, every control step run twice from the same state, every field the library exposes compared bit for bit."""
    import torch
    from tests.test_gpu_fast_chunks import _fields
    from uhc_amd.model.mjcf import self_collision_variant
    from uhc_amd.sim import make_ctrl
    sc = dataclasses.replace(self_collision_variant(model), solver=1)
    c = make_ctrl(sc)
    n = 4
    rng = np.random.default_rng(67)
    qpos = np.tile(standing["qpos"], (n, 1))
    qpos[:, 7:] += rng.normal(scale=0.002, size=(n, 69))
    qpos[:, 2] += np.array([0.0367, 0.04, 0.0433, 0.0467])
    qpos[3], qvel3 = edge_states["qtwo2"], edge_states["vtwo2"]
    qvel = np.zeros((n, sc.nv))
    qvel[3] = qvel3
    tb = torch.from_numpy(qpos[:, 7:].copy()).cuda()
    b = _batch(sc, c, n, path)
    q, v = qpos.copy(), qvel.copy()
    for t in range(4):
        a = torch.from_numpy(rng.normal(scale=0.05, size=(n, c.action_dim))).cuda()
        got = []
        for rep in range(4):
            b.set_state(torch.from_numpy(q), torch.from_numpy(v))
            b.simulate(a, tb)
            b.sync()
            got.append({k: b.field(f).cpu().numpy().copy() for k, f in _fields().items()})
        # Paths 0 and 1 carry nothing over from the step before but the state: EVERY run, the first of a new batch included, gives the first run's words.
        # Under sticky tiers (path 2) the tier an env STARTS the step in is an input too (a function of the tiers and peaks of the steps before), and the words that
        # say which tier did what -- tier, redo, why -- follow it; the tiers compute the same step, so every OTHER word is the first run's from the first run on.  A
        # repeated step settles within two repetitions (large -> general -> fast at most): runs 3 and 4 start every env in the same tier and agree in those three too.
        routing = ("tier", "redo", "why") if path == 2 else ()
        for j in range(1, 4):
            for k in got[j]:
                if k not in routing:
                    assert np.array_equal(got[0][k], got[j][k], equal_nan=True), f"path {path} step {t}: {k} differs between runs 1 and {j + 1} of the same step"
        for k in routing:
            assert np.array_equal(got[2][k], got[3][k], equal_nan=True), f"path {path} step {t}: {k} differs between runs 3 and 4 of the same step"
        q, v = got[3]["qpos"], got[3]["qvel"]
    assert b.give_ups() == 0
