"""GPU: AMASS poses -> qpos rows computed by uhc_smpl_qpos against the host path, `smpl_to_qpose` under the installed scipy, and the env on a bank whose
conversion ran on the device against the env on a bank whose conversion ran on the host.

Inputs, tolerance (1e-9 absolute on every entry) and the conditions asserted on the inputs: tests/smpl_convert_cases.py, the same as the CPU test of the shared
arithmetic (tests/test_smpl_convert_cpu.py).  Host and device differ by the last bits of sqrt / sin / cos / atan2 / hypot; where |cos Y| >= 1e-3 -- asserted --
a relative 1e-15 of the quaternion moves an angle by at most 9.1e-13."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from tests import smpl_convert_cases as K

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
LENGTHS = (1, 2, 3, 63, 64, 65, 129)  # one launch: clips around a wave's 64 lanes (2 2/3 frames), a workgroup's 8 frames, a pair of 99-wide rows; 327 frames: an odd tail
N_LAYOUT = sum(LENGTHS)


@pytest.fixture(scope="module")
def models(model):
    """two body shapes whose root offsets differ visibly"""
    big = dataclasses.replace(model, body_pos=np.asarray(model.body_pos) * 1.1, body_ipos=np.asarray(model.body_ipos) * 1.1)
    assert np.abs(np.asarray(big.body_pos)[1] - np.asarray(model.body_pos)[1]).max() > 1e-3
    return [model, big]


@pytest.fixture(scope="module")
def random_run(models):
    """the 2048 random frames and the edge cases as ONE clip, both outputs from ONE launch; left unchanged"""
    from uhc_amd.sim import smpl_qpos_device
    pose, trans = K.random_poses()
    names, epose, etrans = K.edge_poses()
    rv, npose = K.near_lock_pose()
    all_pose = np.concatenate([pose, epose, npose])
    all_trans = np.concatenate([trans, etrans, np.zeros((1, 3))])
    q, qq = smpl_qpos_device(all_pose, all_trans, [0], models[0], want=("qpos", "qpos_quat"))
    assert q.is_cuda and qq.is_cuda and q.shape == (len(all_pose), 76) and qq.shape == (len(all_pose), 99)
    return dict(pose=all_pose, trans=all_trans, names=names, rv=rv, q=q.cpu().numpy(), qq=qq.cpu().numpy(), n=len(pose), ne=len(names))


def _raw(models, pose, trans, clip_start, clip_model, n_frames, want, count_offset=True, table=None):
    """uhc_smpl_qpos on buffers of this test's own: pre-filled with SENTINEL, one guard row behind the last.  clip_start / clip_model go up as they are."""
    import torch
    from uhc_amd._lib import check, lib
    dev = torch.device("cuda", 0)
    up = lambda x, dt=torch.float64: None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(dev, dt).contiguous()  # noqa: E731
    p, t = up(pose), up(trans)
    cs, cm = up(clip_start, torch.int32), up(clip_model, torch.int32)
    off = up(np.stack([np.asarray(m.body_pos, dtype=np.float64)[1] for m in models])) if count_offset else None
    out = {w: torch.full((n_frames + 1, dict(qpos=76, qpos_quat=99)[w]), SENTINEL, dtype=torch.float64, device=dev) for w in want}
    s2m = np.ascontiguousarray(K.slot_of_joint(models[0])[0] if table is None else table, dtype=np.int32)
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
    check(lib().uhc_smpl_qpos(C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), 24, s2m.ctypes.data_as(C.POINTER(C.c_int32)), ptr(off), len(models), ptr(p), ptr(t),
                              n_frames, ptr(cs), ptr(cm), len(clip_start), ptr(out.get("qpos")), ptr(out.get("qpos_quat"))))
    torch.cuda.synchronize(dev)
    return {w: v.cpu().numpy() for w, v in out.items()}


def test_random_poses_match_the_host_function(random_run, models):
    r = random_run
    n = r["n"]
    branches, margin, cos_y = K.assert_well_conditioned(r["pose"][:n])  # the bars' conditions, asserted on the inputs: nothing is excluded
    assert (branches > 400).all()
    K.assert_rows_match_host(r["q"][:n], r["qq"][:n], r["pose"][:n], r["trans"][:n], models[0])


@pytest.mark.filterwarnings("ignore:Gimbal lock")
def test_named_edge_cases_match_the_host_function(random_run, models):
    r = random_run
    a, b = r["n"], r["n"] + r["ne"]
    K.assert_rows_match_host(r["q"][a:b], r["qq"][a:b], r["pose"][a:b], r["trans"][a:b], models[0], names=r["names"])
    K.assert_lock_rows(r["q"][a:b], r["names"], K.slot_of_joint(models[0])[0])
    K.assert_near_lock_row(r["q"][b], r["rv"])
    zero = r["names"].index("zero")
    assert np.array_equal(r["q"][a + zero, 3:], np.r_[1.0, np.zeros(72)])
    assert np.array_equal(r["qq"][a + zero, 3:], np.tile([1.0, 0.0, 0.0, 0.0], 24))


def test_every_clip_gets_its_own_models_root_offset(random_run, models):
    from uhc_amd.sim import smpl_qpos_device
    from uhc_amd.smpllib.smpl_mujoco import smpl_to_qpose
    pose, trans = random_run["pose"][:N_LAYOUT], random_run["trans"][:N_LAYOUT]
    starts = np.r_[0, np.cumsum(LENGTHS)[:-1]]
    cm = [i % 2 for i in range(len(LENGTHS))]
    q, qq = (x.cpu().numpy() for x in smpl_qpos_device(pose, trans, starts, models, clip_model=cm, want=("qpos", "qpos_quat")))
    for s, T, m in zip(starts, LENGTHS, cm):
        K.assert_rows_match_host(q[s:s + T], qq[s:s + T], pose[s:s + T], trans[s:s + T], models[m])
        other = smpl_to_qpose(pose[s:s + T], models[1 - m], trans=trans[s:s + T])
        assert np.abs(other[:, :3] - q[s:s + T, :3]).max(axis=1).min() > 1e-3  # the other shape's offset is visibly absent from each row
        assert np.abs(other[:, :3] - qq[s:s + T, :3]).max(axis=1).min() > 1e-3
    # everything but the root position is the one-clip launch's, bit for bit: the layout decides the offset and nothing else
    assert np.array_equal(q[:, 3:], random_run["q"][:N_LAYOUT, 3:]) and np.array_equal(qq[:, 3:], random_run["qq"][:N_LAYOUT, 3:])
    # clip_model None: the first shape for every clip
    q0, = smpl_qpos_device(pose, trans, starts, models, want=("qpos",))
    assert np.array_equal(q0.cpu().numpy(), random_run["q"][:N_LAYOUT])


def test_no_trans_and_no_root_offset(random_run, models):
    from uhc_amd.sim import smpl_qpos_device
    pose, trans = random_run["pose"][:70], random_run["trans"][:70]
    q, qq = (x.cpu().numpy() for x in smpl_qpos_device(pose, None, [0], models[0], want=("qpos", "qpos_quat")))
    K.assert_rows_match_host(q, qq, pose, None, models[0])
    assert np.array_equal(q[:, :3], np.tile(np.r_[0.0, 0.0, 0.91437225] + np.asarray(models[0].body_pos)[1], (70, 1)))
    q, qq = (x.cpu().numpy() for x in smpl_qpos_device(pose, trans, [0], models[0], count_offset=False, want=("qpos", "qpos_quat")))
    K.assert_rows_match_host(q, qq, pose, trans, models[0], count_offset=False)
    assert np.array_equal(q[:, :3], trans) and np.array_equal(qq[:, :3], trans)


@pytest.mark.parametrize("n_frames", [1, 8, 64, N_LAYOUT])
def test_rows_are_fully_written_and_the_guard_row_is_untouched(random_run, models, n_frames):
    pose, trans = random_run["pose"][:n_frames], random_run["trans"][:n_frames]
    both = _raw(models, pose, trans, [0], None, n_frames, ("qpos", "qpos_quat"))
    for w, ref in (("qpos", random_run["q"]), ("qpos_quat", random_run["qq"])):
        assert np.array_equal(both[w][n_frames], np.full(both[w].shape[1], SENTINEL)), w  # the guard row
        assert not (both[w][:n_frames] == SENTINEL).any(), w                                # every row, every entry
        assert np.array_equal(both[w][:n_frames], ref[:n_frames]), w                        # ... and what the big launch computed for these frames, bit for bit
    # only one of the two outputs: the same bits, the same guard
    for w in ("qpos", "qpos_quat"):
        one = _raw(models, pose, trans, [0], None, n_frames, (w,))
        assert list(one) == [w] and np.array_equal(one[w], both[w])
    # a second run of the same launch: bit-identical
    again = _raw(models, pose, trans, [0], None, n_frames, ("qpos", "qpos_quat"))
    assert np.array_equal(again["qpos"], both["qpos"]) and np.array_equal(again["qpos_quat"], both["qpos_quat"])


def test_a_clip_table_that_does_not_ascend_names_a_wrong_clip_and_nothing_else(random_run, models):
    """whatever d_clip_start and d_clip_model hold, rows stay whole and in place: only the root offset depends on them, and it is one of the models' (an index
    outside 0 .. n_models - 1 reads as model 0)"""
    n = 100
    pose, trans = random_run["pose"][:n], random_run["trans"][:n]
    got = _raw(models, pose, trans, [90, 40, -5, 2 ** 31 - 1, 7], [1, 7, -3, 0, 1], n, ("qpos", "qpos_quat"))
    offs = [np.asarray(m.body_pos, dtype=np.float64)[1] for m in models]
    for w, ref in (("qpos", random_run["q"]), ("qpos_quat", random_run["qq"])):
        assert np.array_equal(got[w][n], np.full(got[w].shape[1], SENTINEL))
        assert np.array_equal(got[w][:n, 3:], ref[:n, 3:])
        d = [np.abs(got[w][:n, :3] - (trans + o)).max(axis=1) for o in offs]
        assert (np.minimum(d[0], d[1]) == 0.0).all()


def test_single_clip_entry_takes_the_host_functions_arguments(random_run, models):
    from uhc_amd.model.mjcf import ball_variant
    from uhc_amd.smpllib.smpl_mujoco import smpl_to_qpose_device
    pose, trans = random_run["pose"][:33], random_run["trans"][:33]
    q = smpl_to_qpose_device(pose.reshape(33, 24, 3), models[0], trans=trans)
    assert q.is_cuda and np.array_equal(q.cpu().numpy(), random_run["q"][:33])
    qq = smpl_to_qpose_device(pose, ball_variant(models[0]), trans=trans, use_quat=True)
    assert qq.shape == (33, 99) and np.array_equal(qq.cpu().numpy(), random_run["qq"][:33])
    assert smpl_to_qpose_device(np.zeros((0, 72)), models[0]).shape == (0, 76)


# ---------------------------------------------------------------- the env on a device-converted bank
def _clips():
    from uhc_amd.data_loaders.synthetic import make_synthetic_amass
    return {k: dict(pose_aa=v["pose_aa"], trans=v["trans"], beta=np.zeros(16), gender=0) for k, v in make_synthetic_amass(3, seed=7, t_range=(20, 30)).items()}


def _env_run(cfg, clips, convert, n_env):
    import torch
    from uhc_amd.envs.humanoid_im import VecHumanoidEnv
    env = VecHumanoidEnv(cfg, n_env=n_env)
    keys = list(clips.keys())
    env.set_clip_bank(clips, build="device", convert=convert)
    out = dict(bank=env.env._bank[0].cpu().numpy().copy())
    env.assign(np.arange(n_env), [keys[i % len(keys)] for i in range(n_env)], [0, 2, 5, 1][:n_env], [15, 12, 10, 14][:n_env])
    out["obs0"] = env.reset(np.arange(n_env)).cpu().numpy().copy()
    for k in range(3):
        env.step(torch.zeros((n_env, env.action_dim), dtype=torch.float64, device=env.device))
        env.sim.sync()
        out[f"obs{k + 1}"], out[f"reward{k + 1}"] = env.obs.cpu().numpy().copy(), env.reward.cpu().numpy().copy()
    env.close()
    return out


def _assert_same_env(d, h):
    assert d["bank"].shape == h["bank"].shape and np.isfinite(h["bank"]).all()
    np.testing.assert_allclose(d["bank"], h["bank"], atol=1e-8, rtol=0)
    for k in h:
        assert np.isfinite(h[k]).all(), k
        np.testing.assert_allclose(d[k], h[k], atol=1e-8, rtol=0, err_msg=k)


def test_env_on_a_device_converted_bank_matches_the_host_converted_one(tmp_path):
    from uhc_amd.utils.config_utils.copycat_config import Config
    cfg = Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path))
    cfg.env_init_noise = 0.0
    clips = _clips()
    _assert_same_env(_env_run(cfg, clips, "device", 4), _env_run(cfg, clips, "host", 4))


def test_ball_joint_env_on_a_device_converted_bank_matches_too(tmp_path):
    from uhc_amd.utils.config_utils.copycat_config import Config
    cfg = Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path))
    cfg.robot_cfg = {"mesh": True, "model": "smpl", "ball": True}
    cfg.action_type, cfg.residual_force, cfg.meta_pd, cfg.meta_pd_joint = "torque", False, False, False
    cfg.reward_id, cfg.obs_v = "world_rfc_implicit_quat", 2
    cfg.cfg_dict["tq_mul"] = 4
    cfg.env_init_noise = 0.0
    clips = _clips()
    d, h = _env_run(cfg, clips, "device", 2), _env_run(cfg, clips, "host", 2)
    _assert_same_env(d, h)
    np.testing.assert_allclose(d["bank"][:, 3:7], h["bank"][:, 3:7], atol=1e-9, rtol=0)  # the record's root quaternion: the 99-wide rows' [3:7]
