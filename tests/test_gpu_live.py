"""GPU: live targets (uhc_env_live_*): each env imitates a stream of frames appended while it runs.

The stream's records are compared with uhc_expert_frames' of the same rows by EQUALITY: both kernels run the same functions (uhc_expert_math.h), with
contraction off, in the same operation order, on the same math library -- a difference is a bug, not a tolerance.  An env driven by a stream is
compared with an env assigned the same frames as a clip, also by equality: the env kernels are the same and read the same records."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REWARD_W = dict(w_p=0.3, w_v=0.1, w_e=0.45, w_c=0.1, w_vf=0.05, k_p=2.0, k_v=0.005, k_e=5.0, k_c=100.0, k_vf=1.0)
N, CAP = 5, 6  # an odd count: a half wave without a partner, and two waves in one workgroup


def _random_walk(rng, T):
    """A smooth clip: joint steps <= 0.05 rad and root rotation steps <= 0.1 rad per frame (no relative rotation comes near the pi wrap)."""
    from scipy.spatial.transform import Rotation as sRot
    q = np.zeros((T, 76))
    q[:, :3] = np.r_[0.0, 0.0, 0.9] + np.cumsum(rng.uniform(-0.02, 0.02, size=(T, 3)), axis=0)
    r = sRot.from_rotvec(rng.uniform(-1.0, 1.0, size=3))
    for t in range(T):
        step = rng.normal(size=3)
        r = sRot.from_rotvec(step / np.linalg.norm(step) * rng.uniform(0.0, 0.1)) * r
        x, y, z, w = r.as_quat()
        q[t, 3:7] = (w, x, y, z)
    q[:, 7:] = rng.uniform(-0.5, 0.5, size=(1, 69)) + np.cumsum(rng.uniform(-0.05, 0.05, size=(T, 69)), axis=0)
    return q


@pytest.fixture(scope="module")
def models(model):
    from uhc_amd.model.mjcf import scale_model
    return [model, scale_model(model, 1.1)]


@pytest.fixture(scope="module")
def hums(models):
    from uhc_amd.smpllib.torch_smpl_humanoid import Humanoid
    return [Humanoid(model=m) for m in models]


def _batch(models, ctrl, n_env, **desc):
    from uhc_amd import sim as S
    from uhc_amd._capi import env_desc
    ms = list(models) if isinstance(models, (list, tuple)) else [models]
    sb = S.SimBatch(ms, ctrl, n_env)
    return sb, S.EnvBatch(sb, env_desc(ms[0], obs_v=2, reward_v=0, reward_weights=REWARD_W, **desc))


@pytest.fixture(scope="module")
def rig(models, hums, ctrl):
    """Five envs on two body shapes, in live mode; five 6-frame clips and uhc_expert_frames' records of them (computed once, left unchanged)."""
    from uhc_amd.sim import expert_frames_device
    sb, eb = _batch(models, ctrl, N)
    rng = np.random.default_rng(20241020)
    clips = [_random_walk(rng, CAP) for _ in range(N)]
    cm = np.array([e % 2 for e in range(N)])
    want = expert_frames_device(np.concatenate(clips), np.arange(N) * CAP, hums, clip_model=cm).cpu().numpy().reshape(N, CAP, 584)
    yield types.SimpleNamespace(sb=sb, eb=eb, clips=clips, cm=cm, want=want, rng=rng)
    eb.close()
    sb.close()


def _view(eb):
    fr, ln, dr = eb.live_view()
    return fr.cpu().numpy().copy(), ln.cpu().numpy().copy(), dr.cpu().numpy().copy()


def _push_frame(r, t, order):
    import torch
    order = np.ascontiguousarray(order)
    r.eb.live_push(torch.from_numpy(order), np.stack([r.clips[e][t] for e in order]), restart=np.ones(len(order)) if t == 0 else None,
                   model=r.cm[order] if t == 0 else None)


def _begin_clean(r, hums):
    r.eb.live_begin(CAP, hums)


def test_records_equal_the_banks_bit_for_bit(rig, hums):
    _begin_clean(rig, hums)
    for t in range(CAP):
        _push_frame(rig, t, rig.rng.permutation(N))  # ids in a shuffled order that changes per call
    fr, ln, dr = _view(rig.eb)
    assert fr.shape == (N, CAP, 584)
    assert np.array_equal(fr, rig.want), np.abs(fr - rig.want).max()
    assert np.array_equal(fr[:, :, 505:512], np.zeros((N, CAP, 7)))
    assert ln.tolist() == [CAP] * N and dr.tolist() == [0] * N
    # (the two body shapes really differ on this data: a wrong model would show)
    from uhc_amd.sim import expert_frames_device
    other = expert_frames_device(rig.clips[1], [0], hums, clip_model=[0]).cpu().numpy()
    assert np.abs(other[:, 151:223] - rig.want[1][:, 151:223]).max() > 1e-3


def test_frame_zero_alone_is_a_one_frame_clip_then_takes_frame_ones_velocities(rig, hums):
    from uhc_amd.sim import FR, expert_frames_device
    _begin_clean(rig, hums)
    _push_frame(rig, 0, np.arange(N))
    fr, ln, _ = _view(rig.eb)
    one = expert_frames_device(np.stack([c[0] for c in rig.clips]), np.arange(N), hums, clip_model=rig.cm).cpu().numpy()  # N clips of ONE frame
    assert np.array_equal(fr[:, 0], one) and ln.tolist() == [1] * N
    for k in ("qvel", "bangvel"):
        o, n = FR[k]
        assert np.array_equal(fr[:, 0, o:o + n], np.zeros((N, n)))
    assert np.array_equal(fr[:, 1:], np.zeros((N, CAP - 1, 584)))
    _push_frame(rig, 1, np.arange(N)[::-1])
    fr, ln, _ = _view(rig.eb)
    assert ln.tolist() == [2] * N
    for k in ("qvel", "bangvel"):
        o, n = FR[k]
        assert np.array_equal(fr[:, 0, o:o + n], fr[:, 1, o:o + n]) and np.abs(fr[:, 1, o:o + n]).max() > 0
    assert np.array_equal(fr[:, :2], rig.want[:, :2])  # (frames 0 and 1 of a longer clip are those of the two-frame clip)


def test_a_full_stream_an_empty_stream_and_foreign_ids_drop_or_ignore_the_row(rig, hums):
    import torch
    _begin_clean(rig, hums)
    # an append to an env that never restarted is dropped
    rig.eb.live_push(torch.tensor([2]), rig.clips[2][1:2])  # n = 1
    fr, ln, dr = _view(rig.eb)
    assert dr.tolist() == [0, 0, 1, 0, 0] and ln.tolist() == [0] * N and not fr.any()
    for t in range(CAP):
        _push_frame(rig, t, np.arange(N))
    before = _view(rig.eb)
    assert before[2].tolist() == [0] * N  # (the restart cleared env 2's count)
    # a 7th push: the bank unchanged, dropped == 1, the length stays
    rig.eb.live_push(torch.arange(N), np.stack([c[0] for c in rig.clips]) + 0.01)
    fr, ln, dr = _view(rig.eb)
    assert np.array_equal(fr, before[0]) and ln.tolist() == [CAP] * N and dr.tolist() == [1] * N
    # ids -1 and n_env, as appends and as restarts: every array untouched
    cur = [rig.eb.field(f).clone() for f in range(13)]
    for restart in (None, np.ones(2)):
        rig.eb.live_push(torch.tensor([-1, N]), np.stack([rig.clips[0][0], rig.clips[1][0]]) + 0.5, restart=restart, model=None if restart is None else np.array([1, 1]))
    after = _view(rig.eb)
    assert np.array_equal(after[0], before[0]) and after[1].tolist() == [CAP] * N and after[2].tolist() == [1] * N
    assert all(torch.equal(a, b) for a, b in zip(cur, [rig.eb.field(f) for f in range(13)]))


def test_one_call_restarts_one_env_and_appends_to_another(rig, hums):
    import torch
    from uhc_amd.sim import expert_frames_device
    _begin_clean(rig, hums)
    for t in range(3):
        _push_frame(rig, t, np.arange(N))
    before = _view(rig.eb)
    # env 0 starts a new stream with env 4's frame 5 on the OTHER body shape; env 3 gets its frame 3
    rig.eb.live_push(torch.tensor([0, 3]), np.stack([rig.clips[4][5], rig.clips[3][3]]), restart=np.array([1, 0]), model=np.array([1, 0]))
    fr, ln, dr = _view(rig.eb)
    assert ln.tolist() == [1, 3, 3, 4, 3] and dr.tolist() == [0] * N
    assert np.array_equal(fr[0, 0], expert_frames_device(rig.clips[4][5:6], [0], hums, clip_model=[1]).cpu().numpy()[0])
    assert np.array_equal(fr[0, 1:], before[0][0, 1:])  # (the old stream's slots stay as they are: the length says what counts)
    assert np.array_equal(fr[3, :4], rig.want[3, :4]) and not fr[3, 4:].any()  # (d_model of an append is not read: env 3 keeps its shape)
    assert np.array_equal(fr[[1, 2, 4]], before[0][[1, 2, 4]])
    # ... and env 0 goes on from its new frame 0 on its new shape
    rig.eb.live_push(torch.tensor([0]), rig.clips[4][4:5])
    pair = expert_frames_device(np.stack([rig.clips[4][5], rig.clips[4][4]]), [0], hums, clip_model=[1]).cpu().numpy()
    assert np.array_equal(_view(rig.eb)[0][0, :2], pair)


def test_root_quat_record_lands_in_the_record_and_leaves_the_velocities(rig, hums):
    import torch
    from uhc_amd.sim import FR, expert_frames_device
    _begin_clean(rig, hums)
    rq = rig.rng.normal(size=(N, CAP, 4))
    for t in range(CAP):
        rig.eb.live_push(torch.arange(N), np.stack([c[t] for c in rig.clips]), restart=np.ones(N) if t == 0 else None, root_quat_record=rq[:, t],
                         model=rig.cm if t == 0 else None)
    fr, _, _ = _view(rig.eb)
    want = expert_frames_device(np.concatenate(rig.clips), np.arange(N) * CAP, hums, clip_model=rig.cm, root_quat_record=rq.reshape(-1, 4)).cpu().numpy().reshape(N, CAP, 584)
    assert np.array_equal(fr, want)
    assert np.array_equal(fr[:, :, 3:7], rq)
    for k in ("qvel", "bangvel", "wbquat"):
        o, n = FR[k]
        assert np.array_equal(fr[:, :, o:o + n], rig.want[:, :, o:o + n])


def test_live_push_alone_is_captured_and_replayed(rig, hums):
    import torch
    _begin_clean(rig, hums)
    eb, sb = rig.eb, rig.sb
    ids = torch.arange(N, dtype=torch.int32, device="cuda")
    q = torch.zeros(N, 76, dtype=torch.float64, device="cuda")
    rs = torch.zeros(N, dtype=torch.int32, device="cuda")
    md = torch.from_numpy(rig.cm.astype(np.int32)).cuda()
    rows = [torch.from_numpy(np.stack([c[t] for c in rig.clips])).cuda() for t in range(2)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    try:
        with torch.cuda.stream(side):
            sb.use_current_stream()
            eb.live_push(ids, q, restart=rs, model=md)  # (warm-up on the capture stream, as torch asks for: appends to empty streams, all dropped)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                sb.use_current_stream()
                eb.live_push(ids, q, restart=rs, model=md)
            q.copy_(rows[0]); rs.fill_(1)
            g.replay()
            q.copy_(rows[1]); rs.fill_(0)
            g.replay()
            side.synchronize()
    finally:
        sb.use_current_stream()
    fr, ln, dr = _view(eb)
    assert ln.tolist() == [2] * N and dr.tolist() == [0] * N  # (the restart cleared the warm-up's count)
    assert np.array_equal(fr[:, :2], rig.want[:, :2]) and not fr[:, 2:].any()


def test_a_larger_cap_allocates_anew_and_a_smaller_one_reuses_the_memory(rig, hums):
    rig.eb.live_begin(CAP + 3, hums)
    fr, ln, dr = rig.eb.live_view()
    big = fr.data_ptr()
    assert fr.shape == (N, CAP + 3, 584) and not fr.any() and ln.tolist() == [0] * N and dr.tolist() == [0] * N
    for t in range(2):
        _push_frame(rig, t, np.arange(N))
    assert np.array_equal(_view(rig.eb)[0][:, :2], rig.want[:, :2])  # (clip_start follows the new cap)
    rig.eb.live_begin(CAP, hums)
    fr, ln, _ = rig.eb.live_view()
    assert fr.data_ptr() == big and fr.shape == (N, CAP, 584) and not fr.any() and ln.tolist() == [0] * N  # every stream cleared


# ------------------------------------------------------------------ a stream drives the env like a clip
T8 = 8


def _clip_env(model, hums, ctrl, clip, n_env, **desc):
    import torch
    from uhc_amd.sim import expert_frames_device
    sb, eb = _batch(model, ctrl, n_env, **desc)
    eb.set_bank(expert_frames_device(clip, [0], hums[0]), torch.tensor([0], dtype=torch.int32), torch.zeros(1, 17, dtype=torch.float64))
    ids = torch.arange(n_env, dtype=torch.int32)
    eb.assign(ids, torch.zeros(n_env, dtype=torch.int32), torch.zeros(n_env, dtype=torch.int32), torch.full((n_env,), clip.shape[0], dtype=torch.int32))
    eb.reset(ids.cuda(), None)
    return sb, eb


def _live_env(model, hums, ctrl, clip, n_env, head=3, **desc):
    import torch
    sb, eb = _batch(model, ctrl, n_env, **desc)
    eb.live_begin(clip.shape[0], hums[0])
    ids = torch.arange(n_env, dtype=torch.int32)
    for t in range(head):
        eb.live_push(ids, np.tile(clip[t], (n_env, 1)), restart=np.ones(n_env) if t == 0 else None)
    eb.reset(ids.cuda(), None)
    return sb, eb


FIELDS = ("E_OBS", "E_REWARD", "E_REWARD_PARTS", "E_DONE", "E_FAIL", "E_END", "E_TARGET_BASE", "E_CUR_T")


def test_a_stream_drives_the_env_like_a_clip(model, hums, ctrl):
    import torch
    from uhc_amd import sim as S
    n = 3
    rng = np.random.default_rng(7)
    clip = _random_walk(rng, T8)
    acts = torch.from_numpy(rng.normal(scale=0.05, size=(T8 - 1, n, ctrl.action_dim))).cuda()
    sa, ea = _clip_env(model, hums, ctrl, clip, n)
    sb, eb = _live_env(model, hums, ctrl, clip, n)
    ids = torch.arange(n, dtype=torch.int32)
    assert torch.equal(ea.field(S.E_OBS), eb.field(S.E_OBS)) and torch.equal(sa.field(S.F_QPOS), sb.field(S.F_QPOS)) and torch.equal(sa.field(S.F_QVEL), sb.field(S.F_QVEL))
    for t in range(T8 - 1):
        if t + 3 < T8:
            eb.live_push(ids, np.tile(clip[t + 3], (n, 1)))
        ea.step(acts[t].contiguous())
        eb.step(acts[t].contiguous())
        for f in FIELDS:
            assert torch.equal(ea.field(getattr(S, f)), eb.field(getattr(S, f))), (t, f)
        assert torch.equal(sa.field(S.F_QPOS), sb.field(S.F_QPOS)), t
        assert ea.field(S.E_CUR_T).cpu().tolist() == [t + 1] * n
        assert ea.field(S.E_END).cpu().tolist() == [int(t == T8 - 2)] * n  # the clip ends at its last frame, in both, at the same step
    assert torch.equal(ea.field(S.E_PERCENT), eb.field(S.E_PERCENT)) and ea.field(S.E_PERCENT).cpu().tolist() == [1.0] * n
    fr, ln, dr = _view(eb)
    assert ln.tolist() == [T8] * n and dr.tolist() == [0] * n and np.array_equal(fr[0], ea._bank[0].cpu().numpy())
    for x in (ea, eb, sa, sb):
        x.close()


def test_a_stream_that_runs_dry_holds_its_newest_frame_and_ends(model, hums, ctrl):
    import torch
    from uhc_amd import sim as S
    n, trail, last = 3, 2, 4
    clip = _random_walk(np.random.default_rng(8), T8)
    sb, eb = _live_env(model, hums, ctrl, clip, n, env_expert_trail_steps=trail)
    ids = torch.arange(n, dtype=torch.int32)
    act = torch.zeros(n, ctrl.action_dim, dtype=torch.float64, device="cuda")
    for t in range(last + trail):
        if t + 3 <= last:
            eb.live_push(ids, np.tile(clip[t + 3], (n, 1)))  # pushing stops after frame 4
        eb.step(act)
        want = clip[min(t + 1, last), 7:]  # step t aims at frame t + 1; the newest frame stands in for what is not there
        assert np.array_equal(eb.field(S.E_TARGET_BASE).cpu().numpy(), np.tile(want, (n, 1))), t
        assert eb.field(S.E_END).cpu().tolist() == [int(t + 1 >= last + trail)] * n, t  # cur_t = t + 1 >= (len - 1) + trail
    assert eb.live_view()[1].cpu().tolist() == [last + 1] * n
    eb.close()
    sb.close()


def test_calls_that_need_a_window_are_refused_in_live_mode(model, hums, ctrl):
    import torch
    from uhc_amd import sim as S
    from uhc_amd._lib import UhcError
    from uhc_amd.sim import expert_frames_device
    n = 2
    clip = _random_walk(np.random.default_rng(9), T8)
    sb, eb = _live_env(model, hums, ctrl, clip, n)
    ids, z = torch.arange(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
    for call in (lambda: eb.assign(ids, z, z, z + 4), lambda: eb.set_next(ids, z, z, z + 4), lambda: eb.auto_reset(), lambda: eb.set_clip_models(None)):
        with pytest.raises(UhcError, match="live mode"):
            call()
    gen = eb.generation
    eb.live_end()
    with pytest.raises(UhcError, match="no clip bank"):
        eb.step(torch.zeros(n, ctrl.action_dim, dtype=torch.float64, device="cuda"))
    with pytest.raises(UhcError, match="live mode"):
        eb.live_push(ids, np.tile(clip[0], (n, 1)))
    eb.set_bank(expert_frames_device(clip, [0], hums[0]), torch.tensor([0], dtype=torch.int32), torch.zeros(1, 17, dtype=torch.float64))
    assert eb.generation > gen
    eb.assign(ids, z, z, z + T8)  # ... and the env steps from a clip again
    eb.reset(ids.cuda(), None)
    eb.step(torch.zeros(n, ctrl.action_dim, dtype=torch.float64, device="cuda"))
    assert eb.field(S.E_CUR_T).cpu().tolist() == [1] * n
    np.testing.assert_array_equal(eb.field(S.E_TARGET_BASE).cpu().numpy(), np.tile(clip[1, 7:], (n, 1)))
    eb.close()
    sb.close()


# ------------------------------------------------------------------ the env wrapper and the tracker
@pytest.fixture(scope="module")
def amass():
    from uhc_amd.data_loaders.synthetic import make_synthetic_amass
    pk = make_synthetic_amass(2, seed=11, t_range=(6, 7))
    return {k: dict(pose_aa=np.asarray(v["pose_aa"])[:6], trans=np.asarray(v["trans"]).reshape(-1, 3)[:6], beta=np.zeros(16), gender=0) for k, v in pk.items()}


def _venv(tmp_path, n_env):
    from uhc_amd.envs.humanoid_im import VecHumanoidEnv
    from uhc_amd.utils.config_utils.copycat_config import Config
    cfg = Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path))
    cfg.env_init_noise = 0.0
    return VecHumanoidEnv(cfg, n_env=n_env, mode="test")


def test_live_push_smpl_equals_live_push_of_the_converted_rows(tmp_path, amass):
    import torch
    from uhc_amd.sim import smpl_qpos_device
    env = _venv(tmp_path, 2)
    keys = list(amass)
    pose = np.stack([amass[k]["pose_aa"] for k in keys], 1).reshape(6, 2, 72)  # [frame][env]
    trans = np.stack([amass[k]["trans"] for k in keys], 1)
    ids = torch.arange(2, dtype=torch.int32)
    got = []
    for raw in (True, False):
        env.live_begin(6)
        for t in range(6):
            rs = np.ones(2) if t == 0 else None
            if raw:
                env.live_push_smpl(ids, pose[t], trans[t], restart=rs)
            else:
                (rows,) = smpl_qpos_device(pose[t], trans[t], np.arange(2), env.body_models, count_offset=env.cc_cfg.robot_cfg.get("mesh", True))
                env.live_push(ids, rows, restart=rs)
        fr, ln, dr = env.live_view()
        assert ln.cpu().tolist() == [6, 6] and dr.cpu().tolist() == [0, 0]
        got.append(fr.cpu().numpy().copy())
        env.live_end()
    assert np.array_equal(got[0], got[1]) and np.isfinite(got[0]).all() and np.abs(got[0][:, :, 76:151]).max() > 0
    env.close()


def test_stream_tracker_follows_a_stream_as_the_policy_follows_the_clip(tmp_path, amass):
    import torch
    from uhc_amd import sim as S
    from uhc_amd.khrylib.rl.core import PolicyGaussian
    from uhc_amd.khrylib.utils.zfilter import ZFilter
    from uhc_amd.smpllib.smpl_mujoco import smpl_to_qpose
    from uhc_amd.stream import StreamTracker
    n, steps = 2, 4
    keys = list(amass)
    a, b = _venv(tmp_path, n), _venv(tmp_path, n)
    torch.manual_seed(3)
    pol = PolicyGaussian(types.SimpleNamespace(policy_hsize=[64, 32], policy_htype="gelu", fix_std=True, log_std=-2.3), action_dim=a.action_dim, state_dim=a.obs_dim).double().cuda()
    filt = ZFilter((a.obs_dim,), clip=5)
    rng = np.random.default_rng(4)
    filt.set_mean_std(rng.normal(scale=0.1, size=a.obs_dim), rng.uniform(0.5, 2.0, size=a.obs_dim) * 9, 10)  # a frozen filter: (mean, S, n)
    # A: the clips in a bank, built on the device from the host's qpos rows
    a.set_clip_bank(amass, build="device")
    a.assign(np.arange(n), keys, [0, 0], [6, 6])
    a.reset(np.arange(n))
    traj_a = []
    with torch.no_grad():
        for t in range(steps):
            act = pol.select_action(filt(a.obs.to(torch.float64), update=False), True).to(torch.float64).contiguous()
            a.step(act)
            traj_a.append((a.sim.field(S.F_QPOS).clone(), a.done.clone()))
    # B: the same rows as a stream
    rows = np.stack([np.asarray(smpl_to_qpose(pose=amass[k]["pose_aa"], mj_model=b.body_model, trans=amass[k]["trans"], model="smpl",
                                              count_offset=b.cc_cfg.robot_cfg.get("mesh", True)), dtype=np.float64) for k in keys])  # [env][frame][76]
    b.live_begin(6)
    tr = StreamTracker(b, pol, filt)
    obs0 = tr.begin(rows[:, :3])
    assert obs0.shape == (n, b.obs_dim)
    for t in range(steps):
        qpos, done = tr.step(torch.from_numpy(rows[:, t + 3].copy()) if t + 3 < 6 else None)
        assert torch.equal(qpos, traj_a[t][0]) and torch.equal(done, traj_a[t][1]), t
    assert b.live_view()[1].cpu().tolist() == [6] * n
    a.close()
    b.close()


def test_agent_track_stream_follows_a_source_as_its_policy_follows_the_clip(tmp_path):
    """AgentCopycat.track_stream on the agent's own nets: the trajectory is that of the same policy (mean action, frozen filter) on an env that was assigned
    the source's frames as clips of a bank."""
    import torch
    from uhc_amd import sim as S
    from uhc_amd.agents import agent_dict
    from uhc_amd.data_loaders.dataset_amass_single import DatasetAMASSSingle
    from uhc_amd.data_loaders.synthetic import make_synthetic_amass
    from uhc_amd.envs.humanoid_im import VecHumanoidEnv
    from uhc_amd.smpllib.smpl_mujoco import smpl_to_qpose
    from uhc_amd.utils.config_utils.copycat_config import Config
    torch.set_default_dtype(torch.float64)
    cfg = Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path))
    cfg.n_env, cfg.min_batch_size, cfg.num_optim_epoch, cfg.no_log = 2, 16, 1, True
    cfg.policy_hsize = cfg.value_hsize = [64, 32]
    specs = dict(cfg.data_specs)
    specs["file_path"] = "synthetic"
    dl = DatasetAMASSSingle(specs, "train", pickle_data=make_synthetic_amass(2, seed=4, t_range=(12, 14)))
    agent = agent_dict[cfg.agent_name](cfg, torch.float64, torch.device("cuda", 0), data_loader=dl)
    rng = np.random.default_rng(6)
    agent.running_state.set_mean_std(rng.normal(scale=0.1, size=agent.state_dim), rng.uniform(0.5, 2.0, size=agent.state_dim) * 9, 10)
    n, steps, keys = 2, 4, list(dl.data_keys)[:2]
    clips = {k: dict(pose_aa=dl.data["pose_aa"][k], trans=dl.data["trans"][k], beta=np.zeros(16), gender=0) for k in keys}
    rows = [np.asarray(smpl_to_qpose(pose=clips[k]["pose_aa"], mj_model=agent.env.body_model, trans=np.asarray(clips[k]["trans"]).squeeze(), model="smpl",
                                     count_offset=cfg.robot_cfg.get("mesh", True)), dtype=np.float64) for k in keys]
    T = min(r.shape[0] for r in rows)
    assert T >= steps + 3
    src = torch.from_numpy(np.stack([r[:T] for r in rows])).cuda()  # [env][frame][76]
    calls = []

    def source(t):
        calls.append(t)
        return src[:, t].contiguous() if t < T else None

    qpos, ended = agent.track_stream(source, steps)
    assert calls == list(range(steps + 3)) and qpos.shape == (n, steps, agent.env.model.nq) and ended.shape == (n,)
    # the same policy on a bank of the same rows
    ref = VecHumanoidEnv(cfg, n_env=n, mode="test", model=agent.env.body_model)
    ref.set_rfc_rate(agent.env.rfc_rate)
    ref.set_clip_bank(clips, build="device")
    ref.assign(np.arange(n), keys, [0, 0], [T, T])
    ref.reset(np.arange(n))
    with torch.no_grad():
        for t in range(steps):
            ref.step(agent.policy_net.select_action(agent.running_state(ref.obs.to(torch.float64), update=False), True).to(torch.float64).contiguous())
            assert torch.equal(qpos[:, t], ref.sim.field(S.F_QPOS)), t
    assert ended.cpu().tolist() == [steps if not d else steps - 1 for d in ref.done.cpu().tolist()]
    ref.close()
    agent.env.close()
