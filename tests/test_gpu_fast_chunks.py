"""The fast tier's control step in substep chunks (UHC_FAST_CHUNK, uhc_step_kernel<0, 1, *>) computes what the whole-step launch computes, bit for bit.

A chunk boundary is the step's own end-of-step store followed by its own start-of-step load, so nothing may differ: two batches of the same library, one with
UHC_FAST_CHUNK=15 (one chunk: the whole-step launch) and one with a smaller chunk, are stepped side by side and every field the library exposes is compared with
np.array_equal after every control step -- state (qpos, qvel, qacc, body poses), what the next step starts from (qM, qfrc_bias, ctrl, qfrc_applied; the warm start
qacc_warmstart), the counts (ncon, nefc, solver_iter), the flags (fail, overflow, redo, why), the tier decision and the launch-order cost (the only reader of
some of the peaks a step carries across its chunks).  No env-step is left out.

Every case also asserts that no workgroup gave up waiting (uhc_batch_give_ups: queue consumers whose producers never ran beside them, and chunk waiters)."""
import contextlib
import dataclasses
import os

import numpy as np
import pytest

from uhc_amd.sim import REDO_GENERAL, WHY_FAST_SHIFT, WHY_FIELD, WHY_SUBSTEP_SHIFT

pytestmark = pytest.mark.gpu

CHUNKS = (1, 3, 5, 8)
N_SUBSTEPS = 15


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


def _batch(model, ctrl, n, chunk, debug=0):
    from uhc_amd.sim import SimBatch
    with _env(UHC_FAST_CHUNK=chunk, UHC_DEBUG=debug, UHC_FORCE_GENERAL=0):
        return SimBatch(model, ctrl, n)


def _fields():
    from uhc_amd import sim as S
    return dict(qpos=S.F_QPOS, qvel=S.F_QVEL, qacc=S.F_QACC, xpos=S.F_XPOS, xquat=S.F_XQUAT, xipos=S.F_XIPOS, qM=S.F_QM, bias=S.F_QFRC_BIAS, ctrl=S.F_CTRL,
                applied=S.F_QFRC_APPLIED, nefc=S.F_NEFC, ncon=S.F_NCON, solver_iter=S.F_SOLVER_ITER, fail=S.F_FAIL, overflow=S.F_EFC_OVERFLOW, tier=S.F_TIER,
                redo=S.F_REDO, why=S.F_HANDON_WHY, qacc_ws=S.F_QACC_WARMSTART, cost=S.F_COST)


def _assert_same(a, b, where):
    for name, f in _fields().items():
        x, y = a.field(f).cpu().numpy(), b.field(f).cpu().numpy()
        assert np.array_equal(x, y, equal_nan=True), f"{where}: {name} differs in envs {np.unique(np.nonzero(x != y)[0])[:8]}"


def _generated(model):
    from uhc_amd.smpllib.smpl_robot import robot_variant
    return dataclasses.replace(robot_variant(model, {"mesh": True, "model": "smpl"}), solver=1)


def _rollout(ref, new, qpos, qvel, steps, ctrl, seed, tb, path, reset_every=7, act_scale=0.3, where=""):
    """both batches through the same seeded rollout: actions per step, a device-side set_state of a seeded third of the envs every few steps"""
    import torch
    from uhc_amd import sim as S
    rng = np.random.default_rng(seed)
    n = qpos.shape[0]
    for b in (ref, new):
        b.set_kernel_path(path)
        b.set_state(torch.from_numpy(qpos), torch.from_numpy(qvel))
    handed_mid = 0
    for t in range(steps):
        a = torch.from_numpy(rng.normal(scale=act_scale, size=(n, ctrl.action_dim))).cuda()
        if t and t % reset_every == 0:
            ids = np.sort(rng.choice(n, size=max(1, n // 3), replace=False)).astype(np.int32)
            q, v = qpos[ids] + 0.0, rng.normal(scale=0.5, size=(ids.size, qvel.shape[1]))
            q[:, 7:] += rng.normal(scale=0.05, size=(ids.size, qpos.shape[1] - 7))
            for b in (ref, new):
                b.set_state(torch.from_numpy(q), torch.from_numpy(v), env_ids=torch.from_numpy(ids).cuda())
        for b in (ref, new):
            b.simulate(a, tb)
            b.sync()
        _assert_same(ref, new, f"{where} step {t}")
        why, redo = new.field(S.F_HANDON_WHY).cpu().numpy(), new.field(S.F_REDO).cpu().numpy()
        handed_mid += int((((redo & REDO_GENERAL) != 0) & (((why >> WHY_FAST_SHIFT) & WHY_FIELD) != 0) & (((why >> WHY_SUBSTEP_SHIFT) & WHY_FIELD) >= 1)).sum())
    assert int(new.field(S.F_FAIL).sum().item()) == int(ref.field(S.F_FAIL).sum().item())
    return handed_mid


def _states(standing, nq, nv, n, seed, noise=0.1, vel=0.5):
    rng = np.random.default_rng(seed)
    qpos = np.tile(standing["qpos"], (n, 1))
    qpos[:, 7:] += rng.normal(scale=noise, size=(n, nq - 7))
    return qpos, rng.normal(scale=vel, size=(n, nv))


def _drop_states(standing, n, seed=67):
    """the drop scene of test_hand_on_resumes_at_the_substep: self-colliding humanoids 2-7 cm above the floor; the impact takes the rows past 64 in mid-step"""
    rng = np.random.default_rng(seed)
    qpos = np.tile(standing["qpos"], (n, 1))
    qpos[:, 7:] += rng.normal(scale=0.002, size=(n, 69))
    qpos[:, 2] += np.linspace(0.02, 0.07, n)
    return qpos, np.zeros((n, 75))


def _no_giveups(*batches):
    got = [b.give_ups() for b in batches]  # (q_abort: queue consumers and chunk waiters that ran into their 50 ms)
    print("give-ups (whole-step batch, chunked batch):", got)
    assert got == [0] * len(batches), got


@pytest.mark.parametrize("path", [2, 0], ids=["sticky", "chain"])
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("cls", ["generated", "asset"])
def test_chunks_are_bit_equal(model, standing, cls, chunk, path):
    """64 envs, seeded states and actions, 30 control steps with device-side resets in between; the generated (self-colliding) class and the floor-only asset."""
    import torch
    from uhc_amd.sim import make_ctrl
    m = _generated(model) if cls == "generated" else model
    ctrl = make_ctrl(m)
    n = 64
    qpos, qvel = _states(standing, m.nq, m.nv, n, 101)
    tb = torch.from_numpy(qpos[:, 7:].copy()).cuda()
    ref, new = _batch(m, ctrl, n, N_SUBSTEPS), _batch(m, ctrl, n, chunk)
    _rollout(ref, new, qpos, qvel, 30, ctrl, 7, tb, path, where=f"{cls} chunk {chunk}")
    _no_giveups(ref, new)


@pytest.mark.parametrize("path", [2, 0], ids=["sticky", "chain"])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_hand_on_from_a_later_chunk_is_bit_equal(model, standing, chunk, path):
    """The drop scene: the fast tier hands envs on in mid-step, from chunks >= 1 too (asserted from `why`: a hand-on at a substep >= the chunk size)."""
    import torch
    from uhc_amd import sim as S
    from uhc_amd.model.mjcf import self_collision_variant
    from uhc_amd.sim import make_ctrl
    sc = dataclasses.replace(self_collision_variant(model), solver=1)
    ctrl = make_ctrl(sc)
    n = 64
    qpos, qvel = _drop_states(standing, n)
    tb = torch.from_numpy(qpos[:, 7:].copy()).cuda()
    ref, new = _batch(sc, ctrl, n, N_SUBSTEPS), _batch(sc, ctrl, n, chunk)
    a = torch.zeros(n, ctrl.action_dim, dtype=torch.float64, device="cuda")
    for b in (ref, new):
        b.set_kernel_path(path)
        b.set_state(torch.from_numpy(qpos), torch.from_numpy(qvel))
    later = 0
    for t in range(8):
        for b in (ref, new):
            b.simulate(a, tb)
            b.sync()
        _assert_same(ref, new, f"drop chunk {chunk} step {t}")
        why, redo = new.field(S.F_HANDON_WHY).cpu().numpy(), new.field(S.F_REDO).cpu().numpy()
        later += int((((redo & REDO_GENERAL) != 0) & (((why >> WHY_FAST_SHIFT) & WHY_FIELD) != 0) & (((why >> WHY_SUBSTEP_SHIFT) & WHY_FIELD) >= chunk)).sum())
    assert later >= 1, "no env was handed on from a chunk >= 1"
    _no_giveups(ref, new)


@pytest.mark.parametrize("rfc", ["implicit", "explicit"])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_bad_value_at_the_head_of_a_chunk_is_bit_equal(model, standing, chunk, rfc):
    """A bad value found by the check at the HEAD of a substep (qvel beyond 1e10 after the previous substep's Euler step) ends the step before that substep's forward
    pass.  When the substep is the first of a chunk >= 1 the workgroup has run no forward pass of its own: the body poses the step reports are those of the previous
    chunk's last pass, as in the whole-step launch.  Airborne humanoids fly along x at just under 1e10 m/s, each env a little closer to the bound: whichever substep's
    Euler step takes it across, the next head check raises `fail` -- with 1-substep chunks every head is a chunk's, with 3 / 5 / 8 those of substeps 3, 6, ... are.
    A bad-value FLAG, not a fault: the kernels check for it in every substep."""
    import torch
    from uhc_amd import sim as S
    from uhc_amd.sim import make_ctrl
    ctrl = make_ctrl(model, residual_force_mode=rfc)
    n = 64
    qpos, qvel = _states(standing, model.nq, model.nv, n, 57, noise=0.05, vel=0.3)
    qpos[:, 2] += 50.0
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    qvel[:, 0] = sign * (1e10 - np.repeat(np.array([1e-3, 1e-2, 0.1, 1.0, 5.0, 20.0, 100.0, 500.0]), n // 8))
    tb = torch.from_numpy(qpos[:, 7:].copy()).cuda()
    a = torch.from_numpy(np.random.default_rng(3).normal(scale=0.3, size=(n, ctrl.action_dim))).cuda()
    ref, new = _batch(model, ctrl, n, N_SUBSTEPS), _batch(model, ctrl, n, chunk)
    for b in (ref, new):
        b.set_kernel_path(2)
        b.set_state(torch.from_numpy(qpos), torch.from_numpy(qvel))
    head = 0
    for t in range(3):
        for b in (ref, new):
            b.simulate(a, tb)
            b.sync()
        _assert_same(ref, new, f"bad value, {rfc} rfc, chunk {chunk}, step {t}")
        fail, v = ref.field(S.F_FAIL).cpu().numpy(), ref.field(S.F_QVEL).cpu().numpy()
        head = max(head, int(((fail != 0) & (np.abs(v).max(axis=1) > 1e10)).sum()))  # (a stored qvel beyond the bound: the HEAD check of the next substep found it)
    print("envs ended by a head-of-substep check:", head, "of", n)
    assert head >= 4, head
    _no_giveups(ref, new)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_explicit_rfc_is_bit_equal(model, standing, chunk):
    """rfc_mode 2: the residual forces of a substep read the kinematics of the previous forward pass, which cross a chunk boundary through cdof / rootcom /
    xpos / xquat."""
    import torch
    from uhc_amd.sim import make_ctrl
    ctrl = make_ctrl(model, residual_force_mode="explicit")
    n = 64
    qpos, qvel = _states(standing, model.nq, model.nv, n, 31)
    tb = torch.from_numpy(qpos[:, 7:].copy()).cuda()
    ref, new = _batch(model, ctrl, n, N_SUBSTEPS), _batch(model, ctrl, n, chunk)
    _rollout(ref, new, qpos, qvel, 12, ctrl, 9, tb, 2, act_scale=0.2, where=f"explicit rfc chunk {chunk}")
    _no_giveups(ref, new)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_restarts_in_mid_rollout_are_bit_equal(model, ctrl, chunk):
    """uhc_env_auto_reset leaves the forward pass of a restart to the head of the env's next step (DevState::fresh): only chunk 0 runs it, only the step's
    last chunk clears the flag.  Observations, rewards and states of the env layer are bit-equal."""
    import torch
    from uhc_amd import sim as S
    from tests.test_gpu_env import _expert, _make
    expert = _expert()
    beta = np.linspace(-1, 1, 16)
    n = 4
    rng = np.random.default_rng(8)
    noise = torch.from_numpy(rng.normal(scale=0.05, size=(2, model.nu)))
    acts = [torch.from_numpy(rng.normal(scale=0.1, size=(n, ctrl.action_dim))).cuda() for _ in range(7)]
    ids = torch.arange(n, dtype=torch.int32)
    out = []
    for ck in (N_SUBSTEPS, chunk):
        with _env(UHC_FAST_CHUNK=ck, UHC_FORCE_GENERAL=0):
            sb, eb = _make(model, ctrl, n, expert, beta)
        eb.assign(ids, torch.zeros(n, dtype=torch.int32), torch.tensor([0, 4, 0, 8], dtype=torch.int32), torch.tensor([3, 3, 40, 30], dtype=torch.int32))
        eb.reset(ids.cuda(), None)
        eb.set_next(torch.tensor([0], dtype=torch.int32), torch.tensor([1], dtype=torch.int32), torch.tensor([6], dtype=torch.int32), torch.tensor([20], dtype=torch.int32), noise[0:1])
        rec = []
        for t in range(7):
            eb.step(acts[t], None)
            sb.sync()
            rec += [eb.field(S.E_OBS).clone(), eb.field(S.E_REWARD).clone()] + [sb.field(f).clone() for f in _fields().values()]
            if t == 1:
                assert eb.field(S.E_DONE).cpu().tolist() == [1, 1, 0, 0]
                eb.auto_reset()
        assert sb.give_ups() == 0
        out.append(rec)
        sb.close()
    for k, (a, b) in enumerate(zip(*out)):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("chunk", (3, 5))
def test_captured_step_with_chunks_replays_the_eager_step(model, ctrl, standing, chunk):
    """The scene of test_step_inside_a_hip_graph_replays_the_eager_step with chunking on: ticket counter and progress words are reset on the stream inside the
    captured step, so a replay computes the eager step -- here bit for bit against the whole-step launch on the same plain chain."""
    import torch
    n = 32
    qpos, qvel = _states(standing, model.nq, model.nv, n, 23)
    a = torch.from_numpy(np.random.default_rng(5).normal(scale=0.2, size=(n, ctrl.action_dim))).cuda()
    tb = torch.from_numpy(qpos[:, 7:].copy()).cuda()
    eager, graphed = _batch(model, ctrl, n, N_SUBSTEPS), _batch(model, ctrl, n, chunk)
    for bb in (eager, graphed):
        bb.set_kernel_path(0)
        bb.set_state(torch.from_numpy(qpos), torch.from_numpy(qvel))
        bb.sync()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        graphed.use_current_stream()
        graphed.simulate(a, tb)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            graphed.use_current_stream()
            graphed.simulate(a, tb)
        g.replay()
        g.replay()
        side.synchronize()
    for _ in range(3):
        eager.simulate(a, tb)
    eager.sync()
    _assert_same(eager, graphed, f"graph chunk {chunk}")
    _no_giveups(eager, graphed)
