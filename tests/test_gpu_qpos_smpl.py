"""GPU: qpos rows -> SMPL axis-angle poses, translation and 6D rows on the device (uhc_qpos_smpl), the 6D entry (uhc_smpl6d_qpos), and what stands on them:
VecHumanoidEnv.smpl_pose, StreamTracker.step(smpl=True), eval_seqs with eval_smpl.  The references are the host functions (qpos_to_smpl, qpos_quat_to_smpl,
smpl_6d_to_qpose: scipy itself) and the host build of the same arithmetic (tests/smpl_pose_probe.cpp); tolerance 1e-9 absolute on every entry.  Shapes are the
smallest at which the kernel can go wrong: the workgroup edge of 8 rows, odd counts for the 16-byte tails, every row stride its callers have.  Inputs and the
conditions asserted on them: tests/smpl_pose_cases.py."""
import copy
import ctypes as C
import types

import numpy as np
import pytest

from tests import smpl_convert_cases as K
from tests import smpl_pose_cases as P
from tests.test_smpl_pose_cpu import build_probe, probe_rows, probe_rows6d

pytestmark = pytest.mark.gpu
S_ = P.SENTINEL
WIDTHS = dict(pose_aa=72, trans=3, full_6d=147)
COUNTS = (1, 7, 8, 9, 17)


@pytest.fixture(scope="module")
def lib():
    return C.CDLL(build_probe())


@pytest.fixture(scope="module")
def ball_model(model):
    from uhc_amd.model.mjcf import ball_variant
    return ball_variant(model)


@pytest.fixture(scope="module")
def ref(model, ball_model):
    """the host functions on the random rows, once: {ball: (rows, pose_aa, trans, full_6d)}; left unchanged"""
    out = {}
    for ball, m in ((False, model), (True, ball_model)):
        rows = P.random_rows(ball)
        P.assert_well_conditioned(rows, ball)
        pose, trans = P.host_pose_fast(rows, m, ball)
        out[ball] = (rows, pose, trans, P.host_6d(pose, trans))
        for a in out[ball]:
            a.setflags(write=False)
    return out


def _strided(rows, stride, misalign=False):
    """the rows on the device, `stride` doubles apart in a buffer of 5.0 (misalign: the buffer starts 8 bytes behind a 16-byte boundary)"""
    import torch
    n, w = rows.shape
    flat = torch.full((n * stride + 2,), 5.0, dtype=torch.float64, device="cuda")
    assert flat.data_ptr() % 16 == 0
    buf = flat[1:1 + n * stride] if misalign else flat[:n * stride]
    buf = buf.view(n, stride)
    buf[:, :w] = torch.from_numpy(np.array(rows, dtype=np.float64)).cuda()
    return buf


def _outs(n, lead=None):
    import torch
    return {k: torch.full((lead or (n,)) + (w,), S_, dtype=torch.float64, device="cuda") for k, w in WIDTHS.items()}


@pytest.mark.parametrize("stride,ball,misalign", [(76, False, False), (83, False, False), (584, False, False), (76, False, True), (99, True, False), (100, True, False)])
def test_row_counts_strides_and_each_output_alone(model, ball_model, ref, stride, ball, misalign):
    """76 and 584: every row 16-byte aligned (16-byte loads); 83 and 99: odd strides, rows 8-byte aligned only; 76 from a base 8 bytes off: the same by the base;
    100: ball-joint rows with 16-byte loads and the one double behind them"""
    from uhc_amd.sim import qpos_smpl_device
    rows, pose, trans, full = ref[ball]
    want_all = dict(pose_aa=pose, trans=trans, full_6d=full)
    m = ball_model if ball else model
    for n in COUNTS:
        buf = _strided(rows[:n], stride, misalign)
        assert buf.stride(0) == stride and (buf.data_ptr() % 16 == 8) == misalign
        for want in (("pose_aa",), ("trans",), ("full_6d",), ("pose_aa", "trans", "full_6d")):
            out = _outs(n)
            got = qpos_smpl_device(buf, m, want=want, out=out, wait=True)
            assert got[-1] == 0 and len(got) == len(want) + 1
            for k, t in zip(want, got):
                assert t is out[k]
                P.assert_close(t.cpu().numpy(), want_all[k][:n], what=(n, stride, k))
            for k in WIDTHS:  # outputs not asked for are untouched
                if k not in want:
                    assert (out[k] == S_).all(), (n, stride, want, k)
        assert (buf[:, rows.shape[1]:] == 5.0).all()


def test_seq_rows_convert_the_counted_rows_and_leave_the_rest(model, ref):
    import torch
    from uhc_amd.sim import qpos_smpl_device
    rows, pose, trans, full = ref[False]
    counts = [0, 1, 4, 9, -1]  # 9 is clamped to the cap of 4, -1 to 0
    q = torch.from_numpy(rows[:20].reshape(5, 4, 76).copy()).cuda()
    out = _outs(20, lead=(5, 4))
    got = qpos_smpl_device(q, model, seq_rows=torch.tensor(counts, dtype=torch.int32, device="cuda"), want=tuple(WIDTHS), out=out, wait=True)
    assert got[-1] == 0
    live = np.array([[r < min(max(c, 0), 4) for r in range(4)] for c in counts])
    for k, want in (("pose_aa", pose), ("trans", trans), ("full_6d", full)):
        g = out[k].cpu().numpy()
        P.assert_close(g[live], want[:20].reshape(5, 4, -1)[live], what=k)
        assert (g[~live] == S_).all(), k
    # a tensor made by the call: NaN beyond the count
    pose_d, bad = qpos_smpl_device(q, model, seq_rows=torch.tensor(counts, dtype=torch.int32, device="cuda"), want="pose_aa")
    assert np.isnan(pose_d.cpu().numpy()[~live]).all() and int(bad.item()) == 0 and pose_d.shape == (5, 4, 72)


def test_two_models_lose_their_own_root_offset(model, ref):
    import torch
    from uhc_amd.model.mjcf import scale_model
    from uhc_amd.sim import qpos_smpl_device
    rows, pose, trans, full = ref[False]
    ms = [model, scale_model(model, 1.1)]
    off = [np.asarray(m.body_pos)[1] for m in ms]
    assert np.abs(off[0] - off[1]).max() > 1e-3
    n = 9
    sm = np.array([0, 1, 1, 0, 5, -1, 1, 0, 1])  # 5 and -1 are out of range: they read as 0
    eff = np.where((sm < 0) | (sm > 1), 0, sm)
    want = rows[:n, :3] - np.stack([off[i] for i in eff])
    q = torch.from_numpy(rows[:n].copy()).cuda()
    p, t, f, bad = qpos_smpl_device(q, ms, seq_model=torch.tensor(sm, dtype=torch.int32, device="cuda"), want=tuple(WIDTHS), wait=True)
    P.assert_close(t.cpu().numpy(), want, what="trans by model")
    assert torch.equal(f[:, :3], t) and bad == 0
    P.assert_close(p.cpu().numpy(), pose[:n], what="pose_aa")
    t0, _ = qpos_smpl_device(q, ms, want="trans")  # no seq_model: model 0 for every row
    P.assert_close(t0.cpu().numpy(), rows[:n, :3] - off[0], what="trans, model 0")
    t1, f1, _ = qpos_smpl_device(q, ms, seq_model=torch.tensor(sm, dtype=torch.int32, device="cuda"), count_offset=False, want=("trans", "full_6d"))
    assert np.array_equal(t1.cpu().numpy(), rows[:n, :3]) and torch.equal(f1[:, :3], t1)  # no offset at all


@pytest.mark.parametrize("ball", [False, True])
def test_random_and_edge_rows_match_the_host_and_the_probe(lib, model, ball_model, ref, ball):
    import torch
    from uhc_amd.sim import qpos_smpl_device
    m = ball_model if ball else model
    rows, pose, trans, full = ref[ball]
    names, edge = P.edge_rows(ball)
    both = np.concatenate([rows, edge])
    e_pose, e_trans = P.host_pose(edge, m, ball)
    want = dict(pose_aa=np.concatenate([pose, e_pose]), trans=np.concatenate([trans, e_trans]))
    want["full_6d"] = np.concatenate([full, P.host_6d(e_pose, e_trans)])
    labels = [f"random {i}" for i in range(rows.shape[0])] + names
    q = torch.from_numpy(np.array(both)).cuda()
    got = qpos_smpl_device(q, m, want=tuple(WIDTHS), wait=True)
    assert got[-1] == 2  # the zero root quaternion and the NaN triple
    again = qpos_smpl_device(q, m, want=tuple(WIDTHS))
    assert int(again[-1].item()) == 2  # ... and through the device counter
    probe = probe_rows(lib, both, m, ball)
    assert probe[3] == 2
    bad_rows = [rows.shape[0] + names.index(k) for k in P.BAD_NAMES]
    for i, k in enumerate(WIDTHS):
        g = got[i].cpu().numpy()
        P.assert_close(g, want[k], labels, k)
        P.assert_close(g, probe[i], labels, k + " against the host build")
        assert np.isnan(g[bad_rows]).all() and np.isfinite(np.delete(g, bad_rows, axis=0)).all()
        assert np.array_equal(g, again[i].cpu().numpy(), equal_nan=True)
        print(k, "ball" if ball else "hinge", "max |device - host build| =", np.nanmax(np.abs(g - probe[i])), "bit-equal:", np.array_equal(g, probe[i], equal_nan=True))


def test_six_d_in_matches_smpl_6d_to_qpose(lib, model):
    import torch
    from tests.test_smpl_pose_cpu import _six_d_rows
    from uhc_amd.sim import smpl6d_qpos_device
    from uhc_amd.smpllib.smpl_mujoco import smpl_6d_to_qpose, smpl_6d_to_qpose_device
    full, pose, trans = _six_d_rows()
    want = smpl_6d_to_qpose(full[:64], model)
    pq, pqq = probe_rows6d(lib, full[:64], model)
    for n in COUNTS + (64,):  # odd counts: the 99-wide rows end in one 8-byte store
        q, qq = smpl6d_qpos_device(torch.from_numpy(full[:n].copy()).cuda(), [0], model, want=("qpos", "qpos_quat"))
        assert q.shape == (n, 76) and qq.shape == (n, 99)
        assert np.abs(q.cpu().numpy() - want[:n]).max() <= P.TOL
        assert np.abs(q.cpu().numpy() - pq[:n]).max() <= P.TOL and np.abs(qq.cpu().numpy() - pqq[:n]).max() <= P.TOL
    (only,) = smpl6d_qpos_device(full[:9], [0, 4], [model, model], clip_model=[1, 0], count_offset=False, want="qpos_quat")
    assert np.array_equal(only.cpu().numpy()[:, :3], trans[:9]) and np.abs(only.cpu().numpy() - pqq[:9])[:, 3:].max() <= P.TOL
    one = smpl_6d_to_qpose_device(full[:7], model)
    assert np.abs(one.cpu().numpy() - want[:7]).max() <= P.TOL
    # there and back: the 6D rows of the way back are the 6D rows the entry reads
    from uhc_amd.sim import qpos_smpl_device
    f6, bad = qpos_smpl_device(q, model, want="full_6d", wait=True)
    (back,) = smpl6d_qpos_device(f6, [0], model)
    assert bad == 0 and np.abs(back.cpu().numpy() - q.cpu().numpy()).max() <= P.TOL


def test_qpos_to_smpl_device_has_the_host_functions_result(model, ref):
    from uhc_amd.smpllib.smpl_mujoco import qpos_to_smpl_device
    rows, pose, trans, _ = ref[False]
    p, t = qpos_to_smpl_device(rows[:17], model)
    assert p.shape == (17, 24, 3) and t.shape == (17, 3) and p.is_cuda
    P.assert_close(p.cpu().numpy().reshape(17, 72), pose[:17])
    P.assert_close(t.cpu().numpy(), trans[:17])


# ---------------------------------------------------------------- the env, the tracker, eval_seqs
def _cfg(tmp_path, ball=False):
    from uhc_amd.utils.config_utils.copycat_config import Config
    cfg = Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path))
    cfg.env_init_noise = 0.0
    if ball:
        cfg.robot_cfg = {"mesh": True, "model": "smpl", "ball": True}
        cfg.action_type, cfg.residual_force, cfg.meta_pd, cfg.meta_pd_joint = "torque", False, False, False
        cfg.reward_id, cfg.obs_v = "world_rfc_implicit_quat", 2
        cfg.cfg_dict["tq_mul"] = 4
    return cfg


def _clips(objects=0):
    from uhc_amd.data_loaders.synthetic import make_synthetic_amass
    return {k: dict(pose_aa=v["pose_aa"], trans=v["trans"], beta=np.zeros(16), gender=0, obj_pose=v.get("obj_pose"))
            for k, v in make_synthetic_amass(2, seed=7, t_range=(8, 10), objects=objects).items()}


def _host_of_env(env, model_of_env):
    from uhc_amd import sim as S
    from uhc_amd.smpllib.smpl_mujoco import qpos_quat_to_smpl, qpos_to_smpl
    q = env.sim.field(S.F_QPOS).cpu().numpy()
    assert q.shape == (env.n_env, env.qpos_lim + 7 * env.num_obj)
    pose, trans = np.zeros((env.n_env, 72)), np.zeros((env.n_env, 3))
    for e in range(env.n_env):
        p, t = (qpos_quat_to_smpl if env.use_quat else qpos_to_smpl)(q[e:e + 1, :env.qpos_lim], env.body_models[model_of_env[e]])
        pose[e], trans[e] = p.reshape(72), t[0]
    return pose, trans


@pytest.mark.parametrize("kind", ["hinge", "ball", "object", "shapes"])
def test_env_smpl_pose_equals_qpos_to_smpl_of_the_readback(tmp_path, model, kind):
    import torch
    from uhc_amd.envs.humanoid_im import VecHumanoidEnv
    from uhc_amd.model.mjcf import scale_model
    from uhc_amd.model.shapes import box_triangles
    n = 4
    kw = {}
    if kind == "object":
        kw["objects"] = dict(hulls=[box_triangles(0.15, 0.15, 0.15)], density=5.0 / 0.027)
    if kind == "shapes":
        kw["shape_models"] = [scale_model(model, 1.1)]
    env = VecHumanoidEnv(_cfg(tmp_path, ball=kind == "ball"), n_env=n, mode="test", **kw)
    clips = _clips(objects=1 if kind == "object" else 0)
    keys = list(clips)
    env.set_clip_bank(clips, clip_model={keys[0]: 0, keys[1]: 1} if kind == "shapes" else None)
    env.assign(np.arange(n), [keys[i % 2] for i in range(n)], [0, 1, 2, 0], [8, 8, 8, 8])
    model_of_env = [i % 2 if kind == "shapes" else 0 for i in range(n)]
    assert env.sim.field(0).shape[1] == {"hinge": 76, "ball": 99, "object": 83, "shapes": 76}[kind]
    env.reset(np.arange(n))
    held = None
    for steps in (0, 3):
        for _ in range(steps):
            env.step(torch.zeros((n, env.action_dim), dtype=torch.float64, device=env.device))
        pose, trans = env.smpl_pose()
        assert held is None or (pose is held[0] and trans is held[1])  # tensors the env owns and reuses
        held = (pose, trans)
        want_pose, want_trans = _host_of_env(env, model_of_env)
        P.assert_close(pose.cpu().numpy(), want_pose, what=(kind, steps, "pose_aa"))
        P.assert_close(trans.cpu().numpy(), want_trans, what=(kind, steps, "trans"))
    (full,) = env.smpl_pose("full_6d")
    P.assert_close(full.cpu().numpy(), P.host_6d(want_pose, want_trans), what=(kind, "full_6d"))
    if kind == "shapes":
        off = [np.asarray(m.body_pos)[1] for m in env.body_models]
        assert np.abs(off[0] - off[1]).max() > 1e-3 and env.env.field(13).cpu().tolist() == model_of_env
    env.close()


def test_stream_tracker_returns_the_envs_smpl_pose(tmp_path):
    import torch
    from uhc_amd.envs.humanoid_im import VecHumanoidEnv
    from uhc_amd.khrylib.rl.core import PolicyGaussian
    from uhc_amd.smpllib.smpl_mujoco import smpl_to_qpose
    from uhc_amd.stream import StreamTracker
    n = 4
    env = VecHumanoidEnv(_cfg(tmp_path), n_env=n, mode="test")
    clips = _clips()
    keys = list(clips)
    torch.manual_seed(3)
    pol = PolicyGaussian(types.SimpleNamespace(policy_hsize=[64, 32], policy_htype="gelu", fix_std=True, log_std=-2.3), action_dim=env.action_dim, state_dim=env.obs_dim).double().cuda()
    rows = np.stack([np.asarray(smpl_to_qpose(pose=clips[keys[e % 2]]["pose_aa"][:6], mj_model=env.body_model, trans=np.asarray(clips[keys[e % 2]]["trans"]).reshape(-1, 3)[:6],
                                              count_offset=True), dtype=np.float64) for e in range(n)])
    env.live_begin(6)
    tr = StreamTracker(env, pol, None)
    tr.begin(rows[:, :3])
    out = tr.step(torch.from_numpy(rows[:, 3].copy()))
    assert isinstance(out, tuple) and len(out) == 2  # as before
    qpos, done, pose, trans = tr.step(torch.from_numpy(rows[:, 4].copy()), smpl=True)
    assert qpos is out[0] and pose.shape == (n, 72) and trans.shape == (n, 3)
    want_pose, want_trans = _host_of_env(env, [0] * n)
    P.assert_close(pose.cpu().numpy(), want_pose, what="pose_aa")
    P.assert_close(trans.cpu().numpy(), want_trans, what="trans")
    again = env.smpl_pose()
    assert again[0] is pose and again[1] is trans
    env.close()


def test_eval_seqs_hands_back_smpl_parameters_on_both_builds(tmp_path):
    import torch
    from tests.test_gpu_agent import _cfg as agent_cfg
    from uhc_amd.agents import agent_dict
    from uhc_amd.data_loaders.dataset_amass_single import DatasetAMASSSingle
    from uhc_amd.data_loaders.synthetic import make_synthetic_amass
    from uhc_amd.smpllib.smpl_mujoco import qpos_to_smpl
    torch.set_default_dtype(torch.float64)
    cfg = agent_cfg(tmp_path, n_env=4, batch=4 * 4)
    specs = dict(cfg.data_specs)
    specs["file_path"] = "synthetic"
    loader = DatasetAMASSSingle(specs, "train", pickle_data=make_synthetic_amass(2, seed=4, t_range=(8, 12)))
    agent = agent_dict[cfg.agent_name](cfg, torch.float64, torch.device("cuda", 0), data_loader=loader)
    keys = list(loader.data_keys)
    assert len(keys) == 2 and cfg.eval_smpl is False
    rs = agent.running_state.rs
    st = copy.deepcopy(rs.__getstate__())

    def run():  # every pass from the same filter state (eval_seqs filters the reset observation with update=True)
        rs._n = st["_n"]
        rs._M[...], rs._S[...] = st["_M"], st["_S"]
        rs._host_changed()
        return agent.eval_seqs(keys, loader)

    base = run()
    out = {}
    for build in ("host", "device"):
        cfg.eval_build, cfg.eval_smpl = build, False
        off = run()
        assert all(list(off[k]) == list(base[k]) for k in keys) and not any("pose_aa" in name for name in off[keys[0]])  # key off: today's set
        cfg.eval_smpl = True
        out[build] = run()
    cfg.eval_build, cfg.eval_smpl = "host", False
    new = ["pred_pose_aa", "pred_trans", "gt_pose_aa", "gt_trans"]
    for k in keys:
        h, d = out["host"][k], out["device"][k]
        assert set(h) == set(d) == set(base[k]) | set(new)
        T = h["pred"].shape[0]
        for name in new:
            assert h[name].shape == d[name].shape == (T, 72 if "pose" in name else 3), (k, name, h[name].shape, d[name].shape)
        # each build's SMPL parameters are qpos_to_smpl of ITS OWN rows, at the bar; and the two builds agree where their trajectories do
        for res in (h, d):
            for src in ("pred", "gt"):
                pose, trans = qpos_to_smpl(res[src], agent.env.body_model)
                P.assert_close(res[src + "_pose_aa"], pose.reshape(T, 72), what=(k, src))
                P.assert_close(res[src + "_trans"], trans, what=(k, src))
        P.assert_close(d["gt_pose_aa"], h["gt_pose_aa"], what=(k, "gt_pose_aa"))
        P.assert_close(d["gt_trans"], h["gt_trans"], what=(k, "gt_trans"))
        P.assert_close(d["pred_pose_aa"], h["pred_pose_aa"], what=(k, "pred_pose_aa"))
        P.assert_close(d["pred_trans"], h["pred_trans"], what=(k, "pred_trans"))
    for ev in agent._eval_envs.values():
        ev.close()
    agent.env.close()
