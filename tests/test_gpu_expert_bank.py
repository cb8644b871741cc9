"""GPU: the clip bank's frame records computed by uhc_expert_frames against the host path, `pack_expert_frames(Humanoid.qpos_fk(clip))` clip by clip
(Humanoid.qpos_fk itself is pinned to the reference's arrays by tests/golden/g3_qpos_fk.npz).

Tolerance: 1e-9 absolute per entry, tests/test_gpu_env.py's bar for the env layer.  Host and device differ by the last bits of sin / cos / acos; the
worst amplification of those is the acos near +-(1 - 1e-7) -- slope ~2.2e3, times 1 / dt = 30, on a few ulp: ~1e-11."""
import dataclasses
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-9
LENGTHS = (2, 3, 64, 65, 1, 130)  # one launch: clips shorter than, equal to and longer than a workgroup's four frames and a wave's 64 lanes, and ONE frame


def _fields(frames):
    from uhc_amd.sim import FR
    return {k: frames[:, o:o + n] for k, (o, n) in FR.items()}


def _assert_records(got, want, tol=TOL, skip=()):
    assert got.shape == want.shape
    for k, g in _fields(got).items():
        if k not in skip:
            np.testing.assert_allclose(g, _fields(want)[k], atol=tol, rtol=0, err_msg=k)
    np.testing.assert_array_equal(got[:, 505:512], 0.0)  # the slots between com and body_com: zeros, as pack_expert_frames leaves them


def _host(hum, qpos):
    import torch
    from uhc_amd.sim import pack_expert_frames
    return pack_expert_frames(hum.qpos_fk(torch.from_numpy(qpos.copy())))


def _random_walk(rng, T):
    """A smooth clip: joint steps <= 0.05 rad and root rotation steps <= 0.1 rad per frame, so that no relative rotation comes near the pi wrap,
    where host and device could legitimately split."""
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
def hums(model):
    from uhc_amd.smpllib.torch_smpl_humanoid import Humanoid
    big = dataclasses.replace(model, body_pos=np.asarray(model.body_pos) * 1.1, body_ipos=np.asarray(model.body_ipos) * 1.1)
    return [Humanoid(model=model), Humanoid(model=big)]


@pytest.fixture(scope="module")
def walk(hums):
    """Six clips on alternating body shapes, their host records (computed once, left unchanged) and the device's from ONE launch."""
    from uhc_amd.sim import expert_frames_device
    rng = np.random.default_rng(20240607)
    clips = [_random_walk(rng, T) for T in LENGTHS]
    cm = [i % 2 for i in range(len(clips))]
    starts = np.r_[0, np.cumsum(LENGTHS)[:-1]]
    host = [None if T == 1 else _host(hums[m], c) for c, m, T in zip(clips, cm, LENGTHS)]
    dev = expert_frames_device(np.concatenate(clips), starts, hums, clip_model=cm).cpu().numpy()
    return dict(clips=clips, cm=cm, starts=starts, host=host, dev=dev)


def test_golden_clip_matches_the_host_path_and_the_reference_arrays(hums):
    g = np.load(os.path.join(G, "g3_qpos_fk.npz"))
    qpos = g["f_qpos"]
    dev = hums[0].frames_device(qpos).cpu().numpy()
    assert dev.shape == (int(g["f_len"]), 584)
    _assert_records(dev, _host(hums[0], qpos))
    # ... and against the reference's OWN arrays, at tests/test_reference_golden.py::test_expert_features_qpos_fk's tolerance
    for k, v in _fields(dev).items():
        np.testing.assert_allclose(v, g["f_" + k].reshape(v.shape), atol=1e-11, rtol=0, err_msg=k)


def test_every_clip_equals_its_own_host_result_on_its_own_model(walk, hums):
    dev = walk["dev"]
    assert dev.shape == (sum(LENGTHS), 584) and np.isfinite(dev).all()
    for c, m, s, T, h in zip(walk["clips"], walk["cm"], walk["starts"], LENGTHS, walk["host"]):
        rows = dev[s:s + T]
        if T == 1:
            # new ground (the host path cannot pack a clip of one frame): zero velocities, everything else as in a clip that repeats the frame
            f = _fields(rows)
            np.testing.assert_array_equal(f["qvel"], 0.0)
            np.testing.assert_array_equal(f["bangvel"], 0.0)
            _assert_records(rows, _host(hums[m], np.concatenate([c, c]))[:1], skip=("qvel", "bangvel"))
        else:
            _assert_records(rows, h)
            # what a wrong model or a difference across the boundary would look like, measured on THIS data: both are far outside the tolerance
            other = _host(hums[1 - m], c)
            assert np.abs(_fields(other)["wbpos"] - _fields(h)["wbpos"]).max() > 1e-3
    # a difference that reached across a boundary would pair a clip's frame 0 with the previous clip's last frame: on this data that is another
    # velocity by orders of magnitude more than the tolerance (checked here so that the assertion above means something)
    for i in (1, 2, 3, 5):
        s = walk["starts"][i]
        leak = (walk["clips"][i][0, 7:] - walk["clips"][i - 1][-1, 7:]) * 30
        assert np.abs(np.clip(leak, -10, 10) - dev[s, 76 + 6:76 + 75]).max() > 1e-3


def test_frame_zero_takes_frame_ones_velocities(walk):
    from uhc_amd.sim import FR
    for s, T in zip(walk["starts"], LENGTHS):
        if T >= 2:
            for k in ("qvel", "bangvel"):
                o, n = FR[k]
                np.testing.assert_array_equal(walk["dev"][s, o:o + n], walk["dev"][s + 1, o:o + n])


def test_qvel_is_clipped_and_bangvel_is_not(hums):
    rng = np.random.default_rng(5)
    q = _random_walk(rng, 12)
    q[6:, 0] += 0.5       # a jump of 0.5 m in the root position: 15 m/s
    q[6:, 7 + 3 * 4] -= 0.5  # ... and of -0.5 rad in one hinge of body 5: -15 rad/s
    dev = hums[0].frames_device(q).cpu().numpy()
    f = _fields(dev)
    assert f["qvel"][6, 0] == 10.0 and f["qvel"][6, 6 + 3 * 4] == -10.0
    assert np.abs(f["qvel"]).max() == 10.0
    host = _host(hums[0], q)
    _assert_records(dev, host)
    assert np.linalg.norm(f["bangvel"][6, 3 * 5:3 * 5 + 3]) > 12.0  # the body's angular velocity keeps its ~15 rad/s
    np.testing.assert_allclose(f["bangvel"], _fields(host)["bangvel"], atol=TOL, rtol=0)


def test_root_quaternion_override_touches_the_records_quaternion_alone(walk, hums):
    from uhc_amd.sim import expert_frames_device
    qpos = np.concatenate(walk["clips"])
    rng = np.random.default_rng(9)
    over = rng.normal(size=(qpos.shape[0], 4))
    over /= np.linalg.norm(over, axis=1, keepdims=True)
    dev = expert_frames_device(qpos, walk["starts"], hums, clip_model=walk["cm"], root_quat_record=over).cpu().numpy()
    assert np.array_equal(dev[:, 3:7], over)  # bit for bit
    rest = np.r_[0:3, 7:584]
    assert np.array_equal(dev[:, rest], walk["dev"][:, rest])  # kinematics and velocities still read d_qpos' quaternion
    assert np.array_equal(walk["dev"][:, 3:7], qpos[:, 3:7])


def _env_run(cfg, clips, build, n_env=4, step=True):
    import torch
    from uhc_amd import sim as S
    from uhc_amd.envs.humanoid_im import VecHumanoidEnv
    env = VecHumanoidEnv(cfg, n_env=n_env)
    keys = list(clips.keys())
    env.set_clip_bank(clips, build=build)
    out = dict(bank=env.env._bank[0].cpu().numpy().copy())
    if step:
        env.assign(np.arange(n_env), [keys[i % len(keys)] for i in range(n_env)], [0, 2, 5, 1][:n_env], [15, 12, 10, 14][:n_env])
        out["obs0"] = env.reset(np.arange(n_env)).cpu().numpy().copy()
        out["target"] = env.env.field(S.E_TARGET_BASE).cpu().numpy().copy()
        env.step(torch.zeros((n_env, env.action_dim), dtype=torch.float64, device=env.device))
        env.sim.sync()
        out["obs1"], out["reward"] = env.obs.cpu().numpy().copy(), env.reward.cpu().numpy().copy()
    env.close()
    return out


def _clips():
    from uhc_amd.data_loaders.synthetic import make_synthetic_amass
    return {k: dict(pose_aa=v["pose_aa"], trans=v["trans"], beta=np.zeros(16), gender=0) for k, v in make_synthetic_amass(3, seed=7, t_range=(20, 30)).items()}


def test_env_on_a_device_built_bank_matches_the_host_built_one(tmp_path):
    from uhc_amd.utils.config_utils.copycat_config import Config
    cfg = Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path))
    cfg.env_init_noise = 0.0
    clips = _clips()
    h, d = _env_run(cfg, clips, "host"), _env_run(cfg, clips, "device")
    _assert_records(d["bank"], h["bank"])
    assert np.array_equal(d["target"], h["target"])  # the PD target is the expert's qpos, which the kernel copies
    for k in ("obs0", "obs1", "reward"):
        assert np.isfinite(h[k]).all()
        np.testing.assert_allclose(d[k], h[k], atol=1e-8, rtol=0, err_msg=k)


def test_ball_joint_env_bank_carries_the_second_conversions_root_quaternion(tmp_path):
    from uhc_amd.utils.config_utils.copycat_config import Config
    cfg = Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path))
    cfg.robot_cfg = {"mesh": True, "model": "smpl", "ball": True}
    cfg.action_type, cfg.residual_force, cfg.meta_pd, cfg.meta_pd_joint = "torque", False, False, False
    cfg.reward_id, cfg.obs_v = "world_rfc_implicit_quat", 2
    cfg.cfg_dict["tq_mul"] = 4
    cfg.env_init_noise = 0.0
    clips = _clips()
    h, d = _env_run(cfg, clips, "host", n_env=2, step=False), _env_run(cfg, clips, "device", n_env=2, step=False)
    _assert_records(d["bank"], h["bank"])
    assert np.array_equal(d["bank"][:, 3:7], h["bank"][:, 3:7])  # the override is a copy
