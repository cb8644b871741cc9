"""CPU: the way back -- qpos rows -> SMPL axis-angle poses, translation and 6D rows -- and the 6D entry, without a GPU.  (1) the arithmetic of
uhc_amd/csrc/uhc_smpl_convert.h that uhc_smpl.hip computes with, one lane per row and joint, compiled for the host (tests/smpl_pose_probe.cpp, the joints as a plain
loop) against `qpos_to_smpl` / `qpos_quat_to_smpl` / `smpl_6d_to_qpose` under the installed scipy, which is the arbiter, and against the values the reference
recorded; (2) the C-ABI surface of uhc_qpos_smpl and uhc_smpl6d_qpos: declaration, export, ABI version and every argument check, which the library makes BEFORE its
first HIP call; the config key and the Python signatures.  Inputs, tolerance and the asserted input conditions: tests/smpl_pose_cases.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import probe_build
from tests import smpl_convert_cases as K
from tests import smpl_pose_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
FAKE = C.c_void_p(0x1000)  # a non-null, 16-byte aligned "device pointer": every call here is refused or has no rows -- nothing is launched, nothing dereferences it
ODD = C.c_void_p(0x1008)   # 8-byte aligned only


def build_probe(name="smpl_pose_probe"):
    """tests/<name>.cpp + uhc_smpl_convert.h -> uhc_amd/csrc/build/<name>.so with the host compiler: no hipcc, no HIP header."""
    return probe_build.build_probe(name + ".so", ["tests/" + name + ".cpp"], ["uhc_amd/csrc/uhc_smpl_convert.h"], probe_build.NO_CONTRACT)


@pytest.fixture(scope="module")
def probe():
    return C.CDLL(build_probe())


@pytest.fixture(scope="module")
def ball_model(model):
    from uhc_amd.model.mjcf import ball_variant
    return ball_variant(model)


_p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731


def probe_rows(L, rows, mj_model, ball=False, count_offset=True, want=("pose_aa", "trans", "full_6d")):
    """-> (pose_aa, trans, full_6d, bad): None where not asked for"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    n = rows.shape[0]
    off = np.ascontiguousarray(np.asarray(mj_model.body_pos, dtype=np.float64)[1]) if count_offset else None
    _, inv = K.slot_of_joint(mj_model)
    out = [np.full((n, w), P.SENTINEL) if k in want else None for k, w in (("pose_aa", 72), ("trans", 3), ("full_6d", 147))]
    L.uhc_pose_probe_rows.restype = C.c_long
    bad = L.uhc_pose_probe_rows(_p(rows), C.c_long(rows.shape[1]), int(ball), _p(off), _p(inv), C.c_long(n), *[_p(o) for o in out])
    return out[0], out[1], out[2], int(bad)


def probe_rows6d(L, full_6d, mj_model, count_offset=True):
    full_6d = np.ascontiguousarray(full_6d, dtype=np.float64)
    n = full_6d.shape[0]
    off = np.ascontiguousarray(np.asarray(mj_model.body_pos, dtype=np.float64)[1]) if count_offset else None
    _, inv = K.slot_of_joint(mj_model)
    q, qq = np.full((n, 76), P.SENTINEL), np.full((n, 99), P.SENTINEL)
    L.uhc_pose_probe_rows6d(_p(full_6d), _p(off), _p(inv), C.c_long(n), _p(q), _p(qq))
    return q, qq


# ---------------------------------------------------------------- 1. the arithmetic
@pytest.mark.parametrize("ball", [False, True])
def test_probe_matches_the_host_function_on_random_rows(probe, model, ball_model, ball):
    m = ball_model if ball else model
    rows = P.random_rows(ball)
    min_w, lo, hi = P.assert_well_conditioned(rows, ball)  # nothing is excluded below
    assert hi > 3.0 and lo < 0.2 and np.abs(rows[:, 7:76]).max() > np.pi
    assert np.abs(np.linalg.norm(rows[:, 3:7], axis=1) - 1).min() > 1e-6  # non-unit root quaternions
    pose, trans, full, bad = probe_rows(probe, rows, m, ball)
    want_pose, want_trans = P.host_pose_fast(rows, m, ball)
    P.assert_close(pose, want_pose, what="pose_aa")
    P.assert_close(trans, want_trans, what="trans")
    P.assert_close(full, P.host_6d(want_pose, want_trans), what="full_6d")
    assert bad == 0 and np.array_equal(full[:, :3], trans)


@pytest.mark.parametrize("ball", [False, True])
def test_probe_matches_on_the_named_edge_rows_and_counts_the_bad_ones(probe, model, ball_model, ball):
    m = ball_model if ball else model
    names, rows = P.edge_rows(ball)
    assert len(names) == 12
    pose, trans, full, bad = probe_rows(probe, rows, m, ball)
    want_pose, want_trans = P.host_pose(rows, m, ball)
    bad_rows = [names.index(k) for k in P.BAD_NAMES]
    assert sorted(np.nonzero(np.isnan(want_pose).all(axis=1))[0]) == bad_rows  # the host refuses (or spoils) those two rows and no other
    P.assert_close(pose, want_pose, names, "pose_aa")
    P.assert_close(trans, want_trans, names, "trans")
    P.assert_close(full, P.host_6d(want_pose, want_trans), names, "full_6d")
    assert bad == 2
    for out in (pose, trans, full):
        assert np.isnan(out[bad_rows]).all() and np.isfinite(np.delete(out, bad_rows, axis=0)).all()
    assert np.array_equal(pose[names.index("identity")], np.zeros(72))
    i = names.index("w exactly 0")  # not negated: the angle is pi about the axis as it stands
    np.testing.assert_allclose(pose[i, :3], np.pi * rows[i, 4:7], atol=1e-15, rtol=0)
    i = names.index("w < 0")        # negated: the short way round
    np.testing.assert_allclose(np.linalg.norm(pose[i, :3]), 1.1, atol=1e-14, rtol=0)


def test_rotvec_sign_rule_at_w_zero(probe):
    """as_rotvec negates w < 0 and leaves w == 0 (and -0.0) alone"""
    from scipy.spatial.transform import Rotation as sRot
    u = np.array([0.6, -0.3, 0.2]) / np.linalg.norm([0.6, -0.3, 0.2])
    for w in (0.0, -0.0, 1e-300, -1e-300, 1e-12, -1e-12):
        q = np.r_[u * np.sqrt(1 - w * w), w]
        got = np.zeros(3)
        probe.uhc_pose_probe_rotvec(_p(q), _p(got))
        np.testing.assert_allclose(got, sRot.from_quat(q).as_rotvec(), atol=1e-9, rtol=0, err_msg=repr(w))


def test_probe_writes_only_what_is_asked_for_and_skips_the_offset(probe, model):
    rows = P.random_rows()[:8]
    all3 = probe_rows(probe, rows, model)
    for k, name in enumerate(("pose_aa", "trans", "full_6d")):
        got = probe_rows(probe, rows, model, want=(name,))
        assert [g is None for g in got[:3]] == [i != k for i in range(3)] and np.array_equal(got[k], all3[k])
    _, trans, full, _ = probe_rows(probe, rows, model, count_offset=False)
    assert np.array_equal(trans, rows[:, :3]) and np.array_equal(full[:, :3], rows[:, :3])


def test_probe_reads_rows_of_any_stride(probe, model):
    rows = P.random_rows()[:9]
    wide = np.full((9, 83), 5.0)
    wide[:, :76] = rows
    a, b = probe_rows(probe, rows, model), probe_rows(probe, wide, model)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


def test_probe_matches_the_values_recorded_from_the_reference(probe, model):
    g = np.load(os.path.join(G, "g16_boundary_helpers.npz"))
    pose, trans, _, bad = probe_rows(probe, g["qpos"], model)
    np.testing.assert_allclose(pose.reshape(g["pose"].shape), g["pose"], atol=1e-10)  # (tests/test_reference_live.py's tolerances for these arrays)
    np.testing.assert_allclose(trans, g["trans"], atol=1e-13)
    assert bad == 0


def test_6d_out_is_the_float64_form_of_convert_aa_to_orth6d(probe, model):
    from scipy.spatial.transform import Rotation as sRot
    from uhc_amd.data_process.process_amass_db import convert_aa_to_orth6d
    rows = P.random_rows()
    pose, trans, full, _ = probe_rows(probe, rows, model)
    R = sRot.from_rotvec(pose.reshape(-1, 3)).as_matrix()
    d6 = full[:, 3:].reshape(-1, 6)
    assert np.abs(d6[:, :3] - R[:, :, 0]).max() <= P.TOL and np.abs(d6[:, 3:] - R[:, :, 1]).max() <= P.TOL  # column 0, then column 1
    # convert_aa_to_orth6d computes in float32, Rodrigues' formula with the axis as aa / (theta + 1e-6): the axis is short by 1e-6 / theta relative, which enters an
    # entry at most twice; on top a dozen float32 roundings of numbers <= 1 (eps 1.2e-7 each)
    theta = np.linalg.norm(pose.reshape(-1, 3), axis=1)
    f32 = convert_aa_to_orth6d(pose).reshape(-1, 6)
    assert f32.dtype == np.float32
    bound = 2e-6 / theta + 12 * 1.2e-7
    assert (np.abs(f32 - d6.astype(np.float32)) <= bound[:, None]).all(), (np.abs(f32 - d6.astype(np.float32)) / bound[:, None]).max()


def _six_d_rows():
    """6D rows of well-conditioned poses whose two columns are neither unit nor orthogonal: Gram-Schmidt has work to do"""
    pose, trans = K.random_poses()
    K.assert_well_conditioned(pose)
    full = P.host_6d(pose, trans)
    d6 = full[:, 3:].reshape(-1, 6).copy()
    rng = np.random.default_rng(3)
    s, t, u = rng.uniform(0.5, 2.0, size=(3, d6.shape[0], 1))
    a, b = d6[:, :3] * s, d6[:, 3:] * t + (u - 1.0) * d6[:, :3]
    return np.concatenate([trans, np.concatenate([a, b], axis=1).reshape(-1, 144)], axis=1), pose, trans


def test_6d_in_matches_smpl_6d_to_qpose(probe, model):
    from uhc_amd.smpllib.smpl_mujoco import smpl_6d_to_qpose, smpl_to_qpose
    full, pose, trans = _six_d_rows()
    q, qq = probe_rows6d(probe, full, model)
    want = smpl_6d_to_qpose(full, model)
    assert np.abs(q - want).max() <= P.TOL, np.abs(q - want).max()
    assert np.abs(want - smpl_to_qpose(pose, model, trans=trans)).max() <= P.TOL  # (the perturbed columns still name the poses they came from)
    # the 99-wide rows: what the host path gives when the rotation vectors it forms go through smpl_to_qpose(use_quat=True) -- quaternions with w >= 0
    from scipy.spatial.transform import Rotation as sRot
    canon = sRot.from_rotvec(pose.reshape(-1, 3)).as_rotvec().reshape(-1, 72)  # (angles beyond pi folded back, as from_matrix(...).as_rotvec() gives them)
    assert np.abs(qq - smpl_to_qpose(canon, model, trans=trans, use_quat=True)).max() <= P.TOL
    assert (qq[:, 3:].reshape(-1, 4)[:, 0] >= 0).all()
    q0, _ = probe_rows6d(probe, full[:4], model, count_offset=False)
    assert np.array_equal(q0[:, :3], trans[:4])


def test_round_trip_rebuilds_every_rotation(probe, model):
    """smpl_to_qpose o qpos_to_smpl: the qpos rows rebuilt from the probe's poses hold the rotations the rows held, within TOL rad (compared in rotation space, as
    smpl_convert_cases.assert_near_lock_row does: hinge triples beyond +-pi come back wrapped)"""
    from scipy.spatial.transform import Rotation as sRot
    from uhc_amd.smpllib.smpl_mujoco import smpl_to_qpose
    rows = P.random_rows()
    pose, trans, _, _ = probe_rows(probe, rows, model)
    back = smpl_to_qpose(pose, model, trans=trans)
    np.testing.assert_allclose(back[:, :3], rows[:, :3], atol=1e-15, rtol=0)
    d = sRot.from_euler("ZYX", back[:, 7:].reshape(-1, 3)) * sRot.from_euler("ZYX", rows[:, 7:76].reshape(-1, 3)).inv()
    assert d.magnitude().max() <= P.TOL, d.magnitude().max()
    d = sRot.from_quat(back[:, [4, 5, 6, 3]]) * sRot.from_quat(rows[:, [4, 5, 6, 3]]).inv()
    assert d.magnitude().max() <= P.TOL, d.magnitude().max()


def test_host_ball_counterpart_inverts_the_quaternion_conversion(ball_model):
    from scipy.spatial.transform import Rotation as sRot
    from uhc_amd.smpllib.smpl_mujoco import qpos_quat_to_smpl, smpl_to_qpose
    pose, trans = K.random_poses()
    pose, trans = pose[:64], trans[:64]
    back, t = qpos_quat_to_smpl(smpl_to_qpose(pose, ball_model, trans=trans, use_quat=True), ball_model)
    d = sRot.from_rotvec(back.reshape(-1, 3)) * sRot.from_rotvec(pose.reshape(-1, 3)).inv()
    assert d.magnitude().max() <= P.TOL and np.abs(t - trans).max() <= 1e-15


# ---------------------------------------------------------------- 2. the surface
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from uhc_amd import _lib
    return _lib.lib()


ARGS = ["stream", "n_joint", "h_smpl_to_model", "ball", "d_root_offset", "n_models", "d_qpos", "row_stride", "n_seq", "row_cap", "d_seq_rows", "d_seq_model", "d_pose_aa",
        "d_trans", "d_full_6d", "d_bad", "h_bad"]
ARGS6 = ["stream", "n_joint", "h_smpl_to_model", "d_root_offset", "n_models", "d_full_6d", "n_frames", "d_clip_start", "d_clip_model", "n_clips", "d_qpos", "d_qpos_quat"]


def _table():
    from uhc_amd.sim import load_asset_model
    return np.ascontiguousarray(K.slot_of_joint(load_asset_model())[0], dtype=np.int32)


def _call(L, **over):
    a = dict(stream=None, n_joint=24, h_smpl_to_model=_table(), ball=0, d_root_offset=FAKE, n_models=1, d_qpos=FAKE, row_stride=76, n_seq=0, row_cap=1, d_seq_rows=None,
             d_seq_model=None, d_pose_aa=FAKE, d_trans=FAKE, d_full_6d=FAKE, d_bad=FAKE, h_bad=None)
    a.update(over)
    a["h_smpl_to_model"] = None if a["h_smpl_to_model"] is None else a["h_smpl_to_model"].ctypes.data_as(C.POINTER(C.c_int32))
    rc = L.uhc_qpos_smpl(*[a[k] for k in ARGS])
    return rc, L.uhc_last_error().decode()


def _call6(L, **over):
    a = dict(stream=None, n_joint=24, h_smpl_to_model=_table(), d_root_offset=FAKE, n_models=1, d_full_6d=FAKE, n_frames=0, d_clip_start=FAKE, d_clip_model=None, n_clips=1,
             d_qpos=FAKE, d_qpos_quat=FAKE)
    a.update(over)
    a["h_smpl_to_model"] = None if a["h_smpl_to_model"] is None else a["h_smpl_to_model"].ctypes.data_as(C.POINTER(C.c_int32))
    rc = L.uhc_smpl6d_qpos(*[a[k] for k in ARGS6])
    return rc, L.uhc_last_error().decode()


def test_header_declares_both_calls_and_the_abi_is_still_11(L):
    from uhc_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uhc_amd.h")).read(), flags=re.S)
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name, args in (("uhc_qpos_smpl", ARGS), ("uhc_smpl6d_qpos", ARGS6)):
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert re.search(rf" T {name}$", dyn, flags=re.M)
        decl = re.search(rf"\b{name}\s*\((.*?)\);", header, flags=re.S).group(1)  # the declared parameter list is the one this file calls with
        assert [re.search(r"(\w+)\s*$", p).group(1) for p in decl.split(",")] == args
        assert len(getattr(L, name).argtypes) == len(args)
    assert int(re.search(r"#define UHC_ABI_VERSION (\d+)", header).group(1)) == 11
    assert L.uhc_abi_version() == 11


def test_an_empty_call_succeeds_without_a_launch(L):
    assert _call(L)[0] == 0
    h_bad = C.c_int32(-1)
    assert _call(L, h_bad=C.byref(h_bad))[0] == 0 and h_bad.value == 0
    # what may be absent: the root offset (count_offset=False), the row counts, the sequences' models, any two of the three outputs
    assert _call(L, d_root_offset=None, d_seq_rows=FAKE, d_seq_model=FAKE, n_models=3, row_cap=4)[0] == 0
    for keep in ("d_pose_aa", "d_trans", "d_full_6d"):
        assert _call(L, **{k: None for k in ("d_pose_aa", "d_trans", "d_full_6d") if k != keep})[0] == 0
    assert _call(L, ball=1, row_stride=99)[0] == 0 and _call(L, row_stride=83, d_qpos=ODD)[0] == 0 and _call(L, row_stride=584)[0] == 0
    assert _call6(L)[0] == 0
    assert _call6(L, d_root_offset=None, d_clip_model=FAKE, n_models=3, n_clips=5)[0] == 0
    assert _call6(L, d_qpos=None)[0] == 0 and _call6(L, d_qpos_quat=None)[0] == 0


@pytest.mark.parametrize("over,name", [
    (dict(n_joint=23), "n_joint"), (dict(n_joint=52), "n_joint"), (dict(h_smpl_to_model=None), "h_smpl_to_model"), (dict(ball=2), "ball"), (dict(ball=-1), "ball"),
    (dict(d_qpos=None), "d_qpos"), (dict(d_qpos=C.c_void_p(0x1004)), "d_qpos"), (dict(row_stride=75), "row_stride"), (dict(ball=1, row_stride=98), "row_stride"),
    (dict(row_stride=-1), "row_stride"), (dict(row_stride=1 << 32), "row_stride"), (dict(n_seq=-1), "n_seq"), (dict(row_cap=0), "row_cap"), (dict(row_cap=-3), "row_cap"),
    (dict(n_models=0), "n_models"), (dict(n_models=-1), "n_models"),
    (dict(d_pose_aa=None, d_trans=None, d_full_6d=None), "d_pose_aa"), (dict(d_pose_aa=None, d_trans=None, d_full_6d=None), "d_full_6d"),
    (dict(d_pose_aa=ODD), "d_pose_aa"), (dict(d_trans=ODD), "d_trans"), (dict(d_full_6d=ODD), "d_full_6d"), (dict(d_bad=None), "d_bad"),
    (dict(n_seq=1 << 30, row_cap=1 << 30), "row_cap"),
])
def test_bad_arguments_of_qpos_smpl_are_refused_by_name(L, over, name):
    # (n_seq stays 0 where the case does not set it: the checks come before the empty return, and a call that slipped through one would return 0 and fail here
    #  without ever launching on the fake pointers)
    rc, msg = _call(L, **over)
    assert rc != 0 and "uhc_qpos_smpl" in msg and name in msg, (rc, msg)


@pytest.mark.parametrize("over,name", [
    (dict(n_joint=23), "n_joint"), (dict(h_smpl_to_model=None), "h_smpl_to_model"), (dict(d_full_6d=None), "d_full_6d"), (dict(d_clip_start=None), "d_clip_start"),
    (dict(d_qpos=None, d_qpos_quat=None), "d_qpos_quat"), (dict(n_frames=-1), "n_frames"), (dict(n_clips=0), "n_clips"), (dict(n_models=0), "n_models"),
    (dict(d_qpos=ODD), "d_qpos "), (dict(d_qpos_quat=ODD), "d_qpos_quat"), (dict(d_full_6d=C.c_void_p(0x1004)), "d_full_6d"),
])
def test_bad_arguments_of_smpl6d_qpos_are_refused_by_name(L, over, name):
    rc, msg = _call6(L, **over)
    assert rc != 0 and "uhc_smpl6d_qpos" in msg and name in msg, (rc, msg)


def test_a_table_that_is_no_permutation_is_refused_with_its_index(L):
    t = _table()
    for call, fn in ((_call, "uhc_qpos_smpl"), (_call6, "uhc_smpl6d_qpos")):
        for m, j, named in [(0, 1, 0), (1, 0, 1), (5, 24, 5), (5, -1, 5), (7, int(t[3]), 7), (3, int(t[7]), 7), (23, 1000, 23)]:
            bad = t.copy()
            bad[m] = j
            rc, msg = call(L, h_smpl_to_model=bad)
            assert rc != 0 and fn in msg and f"h_smpl_to_model[{named}]" in msg, (m, j, rc, msg)


def test_eval_smpl_defaults_to_false_and_refuses_a_non_bool(tmp_path):
    import yaml
    from uhc_amd.utils.config_utils.copycat_config import Config
    assert Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path)).eval_smpl is False
    shipped = yaml.safe_load(open(os.path.join(ROOT, "config", "uhc_amd", "copycat_mi355x.yml")))
    for value in (True, False):
        assert Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path), cfg_dict=dict(shipped, eval_smpl=value)).eval_smpl is value
    for value in ("yes", 1, "device"):
        with pytest.raises(ValueError, match="eval_smpl"):
            Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path), cfg_dict=dict(shipped, eval_smpl=value))


def test_the_device_entries_have_the_host_functions_signatures(model):
    from uhc_amd.smpllib import smpl_mujoco as M
    for host, dev in ((M.qpos_to_smpl, M.qpos_to_smpl_device), (M.smpl_6d_to_qpose, M.smpl_6d_to_qpose_device)):
        a, b = inspect.signature(host).parameters, inspect.signature(dev).parameters
        assert list(a) == list(b) and all(a[k].default == b[k].default for k in a)
    with pytest.raises(NotImplementedError, match="SMPL-H"):
        M.qpos_to_smpl_device(np.zeros((1, 76)), model, smpl_model="smplh")
    with pytest.raises(NotImplementedError):
        M.smpl_6d_to_qpose_device(np.zeros((1, 147)), model, normalize=True)


def test_the_python_switches_default_to_the_old_behaviour():
    from uhc_amd import eval_ops, sim
    from uhc_amd.envs.humanoid_im import VecHumanoidEnv
    from uhc_amd.stream import StreamTracker
    assert inspect.signature(StreamTracker.step).parameters["smpl"].default is False
    assert inspect.signature(VecHumanoidEnv.smpl_pose).parameters["want"].default == ("pose_aa", "trans")
    assert inspect.signature(sim.qpos_smpl_device).parameters["want"].default == ("pose_aa", "trans")
    assert hasattr(VecHumanoidEnv, "live_push_6d") and hasattr(eval_ops, "smpl_of_record") and hasattr(eval_ops, "smpl_of_bank") and hasattr(sim, "smpl6d_qpos_device")
    with pytest.raises(ValueError, match="want"):
        sim.qpos_smpl_device(None, None, want=("pose",))
