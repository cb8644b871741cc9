"""GPU: endless live streams (uhc_env_live_slide / uhc_env_live_window): a push to a full stream first discards the records behind the frame the env reads next
and moves the others to the front of the env's slice, so a bank of a few frames serves a stream of any length.

The standard is the project's own NON-sliding stream of a large cap on the same rows (tests/test_gpu_live.py ties that one to the clip bank bit for bit): a
sliding env and an unbounded one are driven in lockstep and every comparison is EQUALITY -- the env kernels are the same and must resolve every read to the
same record.  `percent` is the one output left out: under sliding it is cur_t / (len - 1) of the window, by definition."""
import types

import numpy as np
import pytest

from tests import live_window_cases as LW

pytestmark = pytest.mark.gpu
REWARD_W = dict(w_p=0.3, w_v=0.1, w_e=0.45, w_c=0.1, w_vf=0.05, k_p=2.0, k_v=0.005, k_e=5.0, k_c=100.0, k_vf=1.0)
N, BIG, T = 5, 40, 44  # an odd count: the last wave of the append has a half without a partner; the unbounded partner's cap; frames per env
FIELDS = ("E_OBS", "E_REWARD", "E_REWARD_PARTS", "E_DONE", "E_FAIL", "E_END", "E_TARGET_BASE", "E_BODY_DIFF", "E_CUR_T")  # (every env output but E_PERCENT)
# observation v3 with the smallest look-ahead that leaves the window: the post kernel of step t reads frames t + 2 + k skip, the newest pushed one is t + 3
OBS = {"v2": dict(obs_v=2), "v3": dict(obs_v=3, fut_frames=2, fut_skip=2)}


def _random_walk(rng, n_frames):
    """A smooth clip: joint steps <= 0.05 rad and root rotation steps <= 0.1 rad per frame (no relative rotation comes near the pi wrap)."""
    from scipy.spatial.transform import Rotation as sRot
    q = np.zeros((n_frames, 76))
    q[:, :3] = np.r_[0.0, 0.0, 0.9] + np.cumsum(rng.uniform(-0.02, 0.02, size=(n_frames, 3)), axis=0)
    r = sRot.from_rotvec(rng.uniform(-1.0, 1.0, size=3))
    for t in range(n_frames):
        step = rng.normal(size=3)
        r = sRot.from_rotvec(step / np.linalg.norm(step) * rng.uniform(0.0, 0.1)) * r
        x, y, z, w = r.as_quat()
        q[t, 3:7] = (w, x, y, z)
    q[:, 7:] = rng.uniform(-0.5, 0.5, size=(1, 69)) + np.cumsum(rng.uniform(-0.05, 0.05, size=(n_frames, 69)), axis=0)
    return q


@pytest.fixture(scope="module")
def models(model):
    from uhc_amd.model.mjcf import scale_model
    return [model, scale_model(model, 1.1)]


@pytest.fixture(scope="module")
def hums(models):
    from uhc_amd.smpllib.torch_smpl_humanoid import Humanoid
    return [Humanoid(model=m) for m in models]


@pytest.fixture(scope="module")
def data(ctrl):
    """Five random-walk streams on two body shapes and the actions of every step (made once, left unchanged)."""
    import torch
    rng = np.random.default_rng(20241113)
    clips = np.stack([_random_walk(rng, T) for _ in range(N)])  # [env][frame][76]
    acts = torch.from_numpy(rng.normal(scale=0.05, size=(T, N, ctrl.action_dim))).cuda()
    return types.SimpleNamespace(clips=clips, acts=acts, cm=np.array([e % 2 for e in range(N)]), rng=rng)


class Side:
    """One batch of N envs with its env layer."""

    def __init__(self, models, ctrl, **desc):
        from uhc_amd import sim as S
        from uhc_amd._capi import env_desc
        self.sb = S.SimBatch(list(models), ctrl, N)
        self.eb = S.EnvBatch(self.sb, env_desc(models[0], reward_v=0, reward_weights=REWARD_W, **desc))

    def begin(self, hums, cap, slide):
        self.eb.live_begin(cap, hums)
        if slide:
            self.eb.live_slide(True)

    def start(self, d, head):
        """frames 0 .. head - 1 (frame 0 restarts the stream on the env's body shape), then the reset onto frame 0"""
        import torch
        ids = torch.arange(N, dtype=torch.int32)
        for t in range(head):
            self.eb.live_push(ids, d.clips[:, t], restart=np.ones(N) if t == 0 else None, model=d.cm if t == 0 else None)
        self.eb.reset(ids.cuda(), None)

    def push(self, d, t, order=None):
        import torch
        order = np.arange(N) if order is None else np.ascontiguousarray(order)
        self.eb.live_push(torch.from_numpy(order), d.clips[order, t])

    def view(self):
        fr, ln, dr = self.eb.live_view()
        base, moved = self.eb.live_window()
        return types.SimpleNamespace(fr=fr.cpu().numpy().copy(), len=ln.cpu().numpy().copy(), dropped=dr.cpu().numpy().copy(),
                                     base=base.cpu().numpy().copy(), moved=moved.cpu().numpy().copy())

    def close(self):
        self.eb.close()
        self.sb.close()


@pytest.fixture(scope="module")
def sides(models, ctrl):
    """Per observation flavour a pair of batches, (unbounded, sliding), made on first use and always driven in lockstep."""
    made = {}

    def get(obs):
        if obs not in made:
            made[obs] = (Side(models, ctrl, **OBS[obs]), Side(models, ctrl, **OBS[obs]))
        return made[obs]

    yield get
    for pair in made.values():
        for s in pair:
            s.close()


def _same(a, b, where):
    import torch
    from uhc_amd import sim as S
    for f in FIELDS:
        assert torch.equal(a.eb.field(getattr(S, f)), b.eb.field(getattr(S, f))), (where, f)
    for f in ("F_QPOS", "F_QVEL"):
        assert torch.equal(a.sb.field(getattr(S, f)), b.sb.field(getattr(S, f))), (where, f)


def _window_is_the_banks(va, vb):
    """slot i of the sliding env = record base + i of the unbounded bank, bit for bit (slots beyond len are not inspected)"""
    for e in range(N):
        n, b = int(vb.len[e]), int(vb.base[e])
        assert n >= 1 and b + n == va.len[e] and va.base[e] == 0
        assert np.array_equal(vb.fr[e, :n], va.fr[e, b:b + n]), e


def _lockstep(a, b, d, steps, head, t0=0):
    """steps x (push frame t + head in a shuffled order, step with the step's random action), compared after every step"""
    for t in range(t0, t0 + steps):
        order = d.rng.permutation(N)
        for s in (a, b):
            s.push(d, t + head, order)
        for s in (a, b):
            s.eb.step(d.acts[t].contiguous())
        _same(a, b, t)


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("cap", [4, 5, 8])
@pytest.mark.parametrize("obs", ["v2", "v3"])
def test_a_sliding_stream_drives_the_env_like_an_unbounded_one(sides, hums, data, obs, cap):
    from uhc_amd import sim as S
    a, b = sides(obs)
    a.begin(hums, BIG, False)
    b.begin(hums, cap, True)
    for s in (a, b):
        s.start(data, 3)
    _same(a, b, "reset")
    _lockstep(a, b, data, 32, 3)
    va, vb = a.view(), b.view()
    assert a.eb.field(S.E_CUR_T).cpu().tolist() == [32] * N
    assert va.dropped.tolist() == [0] * N and vb.dropped.tolist() == [0] * N
    assert (vb.base + vb.len).tolist() == [35] * N and va.len.tolist() == [35] * N and (vb.len <= cap).all()
    w = LW.session(cap, head=3, steps=32)
    assert vb.base.tolist() == [w.base] * N and vb.moved.tolist() == [w.moved] * N and va.moved.tolist() == [0] * N
    _window_is_the_banks(va, vb)
    assert np.isfinite(a.sb.field(S.F_QPOS).cpu().numpy()).all()


# ------------------------------------------------------------------ 2
def test_the_windows_records_are_the_banks(sides, hums, data):
    a, b = sides("v2")
    a.begin(hums, BIG, False)
    b.begin(hums, 6, True)
    for s in (a, b):
        s.start(data, 3)
    _lockstep(a, b, data, 17, 3)  # 20 pushes
    va, vb = a.view(), b.view()
    assert va.len.tolist() == [20] * N and (vb.base > 0).all() and (vb.base + vb.len).tolist() == [20] * N
    _window_is_the_banks(va, vb)


# ------------------------------------------------------------------ 3
def test_an_overlapping_move(sides, hums, data):
    """cap 8 with the producer 6 frames ahead: a full window has the consumer at slot 2, so S = 2 and records 2 .. 7 go to slots 0 .. 5 through each other."""
    a, b = sides("v2")
    a.begin(hums, BIG, False)
    b.begin(hums, 8, True)
    for s in (a, b):
        s.start(data, 6)
    w = LW.Window(8)
    w.restart()
    for _ in range(5):
        w.push()
    w.reset()
    slides = []
    for t in range(12):
        before = w.base
        w.push()
        slides.append(w.base - before)
        w.step()
        _lockstep(a, b, data, 1, 6, t0=t)
        _window_is_the_banks(a.view(), b.view())
    assert set(slides) == {0, 2} and slides.count(2) >= 4  # (every slide is by 2 out of 8: source and destination overlap)
    vb = b.view()
    assert vb.moved.tolist() == [w.moved] * N and vb.base.tolist() == [w.base] * N and vb.len.tolist() == [w.len] * N and vb.dropped.tolist() == [0] * N


# ------------------------------------------------------------------ 4
def test_a_full_window_with_an_idle_consumer_still_drops(sides, hums, data):
    a, b = sides("v2")
    for s in (a, b):
        s.begin(hums, BIG if s is a else 4, s is b)
        s.start(data, 3)
        s.push(data, 3)  # the sliding window is full now, and its env has not stepped
    before = b.view()
    assert before.len.tolist() == [4] * N
    b.push(data, 4)
    after = b.view()
    assert after.dropped.tolist() == [1] * N and after.len.tolist() == [4] * N and after.base.tolist() == [0] * N and after.moved.tolist() == [0] * N
    assert np.array_equal(after.fr, before.fr)
    for s in (a, b):  # ... and the env reads what it read: one step beside the unbounded env, which never saw the dropped row
        s.eb.step(data.acts[0].contiguous())
    _same(a, b, "after the drop")


# ------------------------------------------------------------------ 5
def test_a_dry_stream_slides_down_to_its_newest_frame_which_keeps_its_velocities(sides, hums, data):
    from uhc_amd import sim as S
    from uhc_amd.sim import FR
    a, b = sides("v2")
    a.begin(hums, BIG, False)
    b.begin(hums, 4, True)
    for s in (a, b):
        s.start(data, 3)
    _lockstep(a, b, data, 2, 3)  # frames 3 and 4, cur_t = 2
    ends = []
    for t in range(2, 6):  # no push: the newest frame (4) is held, `end` rises at cur_t = 4
        for s in (a, b):
            s.eb.step(data.acts[t].contiguous())
        _same(a, b, ("dry", t))
        ends.append(a.eb.field(S.E_END).cpu().tolist())
        assert np.array_equal(b.eb.field(S.E_TARGET_BASE).cpu().numpy(), data.clips[:, min(t + 1, 4), 7:]), t  # step t aims at frame t + 1
    assert ends == [[0] * N, [1] * N, [1] * N, [1] * N]
    vb = b.view()
    assert vb.len.tolist() == [4] * N and vb.base.tolist() == [1] * N
    frame4 = vb.fr[:, 3].copy()
    # three more rows: the first push slides the window down to the newest frame alone, then appends
    for k, t in enumerate(range(6, 9)):
        for s in (a, b):
            s.push(data, t - 1)  # frames 5, 6, 7
        va, vb = a.view(), b.view()
        if k == 0:
            assert vb.len.tolist() == [2] * N and vb.base.tolist() == [4] * N and vb.moved.tolist() == [3 + 1] * N
            assert np.array_equal(vb.fr[:, 0], frame4)  # slot 0 is frame 4 as it was: local frame 1 did not hand it its velocities
            for name in ("qvel", "bangvel"):
                o, n = FR[name]
                assert np.array_equal(vb.fr[:, 0, o:o + n], va.fr[:, 4, o:o + n]) and not np.array_equal(vb.fr[:, 0, o:o + n], vb.fr[:, 1, o:o + n])
        _window_is_the_banks(va, vb)
        for s in (a, b):
            s.eb.step(data.acts[t].contiguous())
        _same(a, b, ("fed again", t))
    assert b.view().dropped.tolist() == [0] * N


# ------------------------------------------------------------------ 6
def test_one_call_with_mixed_rows_equals_the_single_row_calls(sides, hums, data):
    import torch
    from uhc_amd import sim as S
    a, b = sides("v2")
    rows = {0: data.clips[0, 5], 1: data.clips[1, 3], 3: data.clips[2, 9], N + 3: data.clips[4, 0] + 0.5}
    restart, model = {0: 0, 1: 0, 3: 1, N + 3: 0}, {0: 0, 1: 0, 3: 0, N + 3: 1}  # env 3 (shape 1) restarts on shape 0
    for s in (a, b):
        s.begin(hums, 4, True)
        s.start(data, 3)
        for t in (0, 1):  # envs 0, 2, 3, 4 get frames 3 and 4: full, and slid once; env 1 holds three frames
            s.eb.live_push(torch.tensor([0, 2, 3, 4]), data.clips[[0, 2, 3, 4], t + 3])
            s.eb.step(data.acts[t].contiguous())
    before = b.view()
    assert before.len.tolist() == [4, 3, 4, 4, 4] and before.base.tolist() == [1, 0, 1, 1, 1] and before.moved.tolist() == [3, 0, 3, 3, 3]
    fields_before = [b.eb.field(f).clone() for f in range(14)]
    # a: one call, ids shuffled -- the restart, the foreign id, the slide, the plain append; envs 2 and 4 are absent
    ids = [3, N + 3, 0, 1]
    a.eb.live_push(torch.tensor(ids), np.stack([rows[i] for i in ids]), restart=np.array([restart[i] for i in ids]), model=np.array([model[i] for i in ids]))
    # b: one call per row
    for i in (0, 1, 3, N + 3):
        b.eb.live_push(torch.tensor([i]), rows[i][None], restart=np.array([restart[i]]), model=np.array([model[i]]))
    va, vb = a.view(), b.view()
    for k in ("fr", "len", "dropped", "base", "moved"):
        assert np.array_equal(getattr(va, k), getattr(vb, k)), k
    for f in range(14):
        assert torch.equal(a.eb.field(f), b.eb.field(f)), f
    # env 0 slid again and appended; env 1 appended; env 3 restarted: base and moved are back to 0; envs 2 and 4 stay as they were
    assert va.len.tolist() == [4, 4, 4, 1, 4] and va.base.tolist() == [2, 0, 1, 0, 1] and va.moved.tolist() == [6, 0, 3, 0, 3] and va.dropped.tolist() == [0] * N
    assert a.eb.field(S.E_MODEL).cpu().tolist() == [0, 1, 0, 0, 0]
    assert np.array_equal(va.fr[0, :3], before.fr[0, 1:4])  # env 0 slid by one ...
    assert np.array_equal(va.fr[[2, 4]], before.fr[[2, 4]])  # ... the absent envs did not, full as they are
    for f in range(13):  # the push writes no env output; of the env's arrays only the listed envs' bookkeeping moved
        assert torch.equal(b.eb.field(f), fields_before[f]), f
    for s in (a, b):  # the restarted env is reset, and the batch steps on as one
        s.eb.reset(torch.tensor([3], dtype=torch.int32).cuda(), None)
        s.eb.step(data.acts[2].contiguous())
    _same(a, b, "after the mixed call")
    assert a.eb.field(S.E_CUR_T).cpu().tolist() == [3, 3, 3, 1, 3]


# ------------------------------------------------------------------ 7
def test_a_captured_push_slides_at_every_replay_that_has_to(sides, hums, data):
    import torch
    a, b = sides("v2")  # a: eager; b: one captured live_push, replayed with its inputs rewritten in place
    for s in (a, b):
        s.begin(hums, 4, True)
    ids = torch.arange(N, dtype=torch.int32, device="cuda")
    q = torch.zeros(N, 76, dtype=torch.float64, device="cuda")
    rs = torch.zeros(N, dtype=torch.int32, device="cuda")
    md = torch.from_numpy(data.cm.astype(np.int32)).cuda()
    rows = torch.from_numpy(data.clips).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    try:
        with torch.cuda.stream(side):
            b.sb.use_current_stream()
            b.eb.live_push(ids, q, restart=rs, model=md)  # (warm-up on the capture stream, as torch asks for: appends to empty streams, all dropped)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                b.sb.use_current_stream()
                b.eb.live_push(ids, q, restart=rs, model=md)
            side.synchronize()
    finally:
        b.sb.use_current_stream()
    # (the replays and the steps between them share the current stream)
    for t in range(3):
        q.copy_(rows[:, t]); rs.fill_(1 if t == 0 else 0)
        g.replay()
        a.eb.live_push(ids, rows[:, t].contiguous(), restart=rs.clone(), model=md)
    for s in (a, b):
        s.eb.reset(ids, None)
    for t in range(6):
        q.copy_(rows[:, t + 3]); rs.fill_(0)
        g.replay()
        a.eb.live_push(ids, rows[:, t + 3].contiguous(), restart=rs.clone(), model=md)
        for s in (a, b):
            s.eb.step(data.acts[t].contiguous())
        _same(a, b, t)
    va, vb = a.view(), b.view()
    for k in ("fr", "len", "dropped", "base", "moved"):
        assert np.array_equal(getattr(va, k), getattr(vb, k)), k
    assert vb.base.tolist() == [5] * N and vb.len.tolist() == [4] * N and vb.moved.tolist() == [15] * N and vb.dropped.tolist() == [0] * N  # five slide boundaries


# ------------------------------------------------------------------ 8
def test_sliding_is_off_by_default_and_refused_where_it_cannot_hold(sides, hums, data, model, ctrl):
    import torch
    from uhc_amd import sim as S
    from uhc_amd._capi import env_desc
    from uhc_amd._lib import UhcError
    a, b = sides("v2")
    # off after live_begin -- also after a live_begin that follows a sliding session: a full stream drops the row although its env has moved on
    b.begin(hums, 4, True)
    b.begin(hums, 4, False)
    a.begin(hums, BIG, False)
    for s in (a, b):
        s.start(data, 3)
    _lockstep(a, b, data, 1, 3)
    before = b.view()
    b.push(data, 4)
    after = b.view()
    assert after.dropped.tolist() == [1] * N and after.len.tolist() == [4] * N and after.base.tolist() == [0] * N and np.array_equal(after.fr, before.fr)
    # switched on now, the stream goes on from the next row; switched off after slides, the window stays readable and the next full push drops
    b.eb.live_slide(True)
    a.push(data, 4)
    b.push(data, 4)
    for s in (a, b):
        s.eb.step(data.acts[1].contiguous())
    _same(a, b, "switched on")
    _lockstep(a, b, data, 3, 3, t0=2)
    b.eb.live_slide(False)
    before = b.view()
    assert before.base.tolist() == [4] * N and before.len.tolist() == [4] * N
    b.push(data, 8)
    after = b.view()
    assert after.dropped.tolist() == [2] * N and after.base.tolist() == [4] * N and np.array_equal(after.fr, before.fr)
    for s in (a, b):
        s.eb.step(data.acts[5].contiguous())
    _same(a, b, "switched off")
    _window_is_the_banks(a.view(), after)
    # outside live mode
    b.eb.live_end()
    for call in (lambda: b.eb.live_slide(True), lambda: b.eb.live_slide(False), lambda: b.eb.live_window()):
        with pytest.raises(UhcError, match="not in live mode"):
            call()
    # observation v0 with the phase word: cur_t / len would jump at a slide
    sb = S.SimBatch(model, ctrl, 2)
    for phase in (True, False):
        eb = S.EnvBatch(sb, env_desc(model, obs_v=0, reward_v=0, reward_weights=REWARD_W, obs_phase=phase))
        eb.live_begin(4, hums[0])
        if phase:
            with pytest.raises(UhcError, match="uhc_env_live_slide.*phase word"):
                eb.live_slide(True)
            eb.live_slide(False)  # (switching off is always possible)
        else:
            eb.live_slide(True)
        assert torch.equal(eb.live_window()[0], torch.zeros(2, dtype=torch.int32, device="cuda"))
        eb.close()
    sb.close()


# ------------------------------------------------------------------ 9
def test_track_stream_in_a_window_of_six_frames_equals_track_stream(tmp_path):
    import torch
    from uhc_amd.agents import agent_dict
    from uhc_amd.data_loaders.dataset_amass_single import DatasetAMASSSingle
    from uhc_amd.data_loaders.synthetic import make_synthetic_amass
    from uhc_amd.smpllib.smpl_mujoco import smpl_to_qpose
    from uhc_amd.utils.config_utils.copycat_config import Config
    torch.set_default_dtype(torch.float64)
    cfg = Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path))
    cfg.n_env, cfg.min_batch_size, cfg.num_optim_epoch, cfg.no_log = 4, 16, 1, True
    cfg.policy_hsize = cfg.value_hsize = [64, 32]
    specs = dict(cfg.data_specs)
    specs["file_path"] = "synthetic"
    dl = DatasetAMASSSingle(specs, "train", pickle_data=make_synthetic_amass(4, seed=4, t_range=(30, 32)))
    agent = agent_dict[cfg.agent_name](cfg, torch.float64, torch.device("cuda", 0), data_loader=dl)
    rng = np.random.default_rng(6)
    agent.running_state.set_mean_std(rng.normal(scale=0.1, size=agent.state_dim), rng.uniform(0.5, 2.0, size=agent.state_dim) * 9, 10)
    n, steps, keys = 4, 24, list(dl.data_keys)[:4]
    rows = [np.asarray(smpl_to_qpose(pose=dl.data["pose_aa"][k], mj_model=agent.env.body_model, trans=np.asarray(dl.data["trans"][k]).squeeze(), model="smpl",
                                     count_offset=cfg.robot_cfg.get("mesh", True)), dtype=np.float64) for k in keys]
    n_frames = min(r.shape[0] for r in rows)
    assert n_frames >= steps + 3
    src = torch.from_numpy(np.stack([r[:n_frames] for r in rows])).cuda()  # [env][frame][76]

    def source(t):
        return src[:, t].contiguous() if t < n_frames else None

    qpos, ended = agent.track_stream(source, steps, n_env=n)
    ev = agent._stream_envs[n]
    qpos6, ended6 = agent.track_stream(source, steps, n_env=n, cap=6)
    assert qpos.shape == (n, steps, agent.env.model.nq) and torch.isfinite(qpos).all()
    assert torch.equal(qpos6, qpos) and torch.equal(ended6, ended)
    assert agent._stream_envs[n] is ev  # (the same env served both runs: its bank was 28 frames a stream, then a window of 6)
    agent.env.close()
