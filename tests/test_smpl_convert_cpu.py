"""CPU: the AMASS -> qpos conversion of the device path without a GPU.  (1) uhc_amd/csrc/uhc_smpl_convert.h -- the per-joint arithmetic uhc_smpl.hip computes with, one
lane per frame and joint -- compiled for the host (tests/smpl_convert_probe.cpp, the joints as a plain loop) against `smpl_to_qpose` under the installed scipy, which
is the arbiter, and against the values the reference recorded; (2) the C-ABI surface of uhc_smpl_qpos: declaration, export, ABI version and every argument check,
which the library makes BEFORE its first HIP call; the config key and the Python switches.  Inputs, tolerance and the asserted input conditions:
tests/smpl_convert_cases.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import probe_build
from tests import smpl_convert_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
SENTINEL = -7.0
FAKE = C.c_void_p(0x1000)  # a non-null, 16-byte aligned "device pointer": every call here is refused or has n_frames == 0 -- nothing is launched, nothing dereferences it


def build_probe():
    """tests/smpl_convert_probe.cpp + uhc_smpl_convert.h -> uhc_amd/csrc/build/smpl_convert_probe.so with the host compiler: no hipcc, no HIP header."""
    return probe_build.build_probe("smpl_convert_probe.so", ["tests/smpl_convert_probe.cpp"], ["uhc_amd/csrc/uhc_smpl_convert.h"], probe_build.NO_CONTRACT)


@pytest.fixture(scope="module")
def probe():
    return C.CDLL(build_probe())


def probe_rows(P, pose, trans, mj_model, count_offset=True, want=("qpos", "qpos_quat")):
    """-> (qpos or None, qpos_quat or None), SENTINEL where the probe wrote nothing"""
    pose = np.ascontiguousarray(pose, dtype=np.float64).reshape(-1, 72)
    n = pose.shape[0]
    trans = None if trans is None else np.ascontiguousarray(trans, dtype=np.float64).reshape(n, 3)
    off = np.ascontiguousarray(np.asarray(mj_model.body_pos, dtype=np.float64)[1]) if count_offset else None
    _, inv = K.slot_of_joint(mj_model)
    q = np.full((n, 76), SENTINEL) if "qpos" in want else None
    qq = np.full((n, 99), SENTINEL) if "qpos_quat" in want else None
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    P.uhc_smpl_probe_rows(p(pose), p(trans), p(off), p(inv), C.c_long(n), p(q), p(qq))
    return q, qq


# ---------------------------------------------------------------- 1. the arithmetic
def test_probe_matches_smpl_to_qpose_on_random_poses(probe, model):
    pose, trans = K.random_poses()
    branches, margin, cos_y = K.assert_well_conditioned(pose)  # zero joints with |cos Y| < 1e-3, branch margin > 1e-6: nothing is excluded below
    assert (branches > 400).all(), branches                    # every branch of the root quaternion occurs, hundreds of times
    assert np.linalg.norm(pose.reshape(-1, 3), axis=1).max() > 2 * np.pi
    q, qq = probe_rows(probe, pose, trans, model)
    K.assert_rows_match_host(q, qq, pose, trans, model)
    assert not (q == SENTINEL).any() and not (qq == SENTINEL).any()


def test_probe_matches_without_trans_and_without_the_root_offset(probe, model):
    pose, trans = K.random_poses()
    pose, trans = pose[:16], trans[:16]
    q, qq = probe_rows(probe, pose, None, model)
    K.assert_rows_match_host(q, qq, pose, None, model)
    assert np.array_equal(q[:, :3], np.tile(np.r_[0.0, 0.0, 0.91437225] + np.asarray(model.body_pos)[1], (16, 1)))
    q, qq = probe_rows(probe, pose, trans, model, count_offset=False)
    K.assert_rows_match_host(q, qq, pose, trans, model, count_offset=False)
    assert np.array_equal(q[:, :3], trans) and np.array_equal(qq[:, :3], trans)


def test_probe_writes_only_the_rows_asked_for(probe, model):
    pose, trans = K.random_poses()
    both = probe_rows(probe, pose[:8], trans[:8], model)
    q, none = probe_rows(probe, pose[:8], trans[:8], model, want=("qpos",))
    assert none is None and np.array_equal(q, both[0])
    none, qq = probe_rows(probe, pose[:8], trans[:8], model, want=("qpos_quat",))
    assert none is None and np.array_equal(qq, both[1])


@pytest.mark.filterwarnings("ignore:Gimbal lock")
def test_probe_matches_on_the_named_edge_cases(probe, model):
    names, pose, trans = K.edge_poses()
    assert {"zero", "1e-3 exactly", "just below 1e-3", "just above 1e-3", "1e-8", "beyond 2 pi", "lock +pi/2", "lock -pi/2"} == set(names)
    q, qq = probe_rows(probe, pose, trans, model)
    K.assert_rows_match_host(q, qq, pose, trans, model, names=names)
    K.assert_lock_rows(q, names, K.slot_of_joint(model)[0])
    zero = q[names.index("zero")]
    assert np.array_equal(zero[3:], np.r_[1.0, np.zeros(72)])  # the identity: root quaternion (1, 0, 0, 0), every angle 0
    assert np.array_equal(qq[names.index("zero"), 3:], np.tile([1.0, 0.0, 0.0, 0.0], 24))


def test_probe_euler_triple_near_lock_is_the_same_rotation(probe, model):
    rv, pose = K.near_lock_pose()
    q, _ = probe_rows(probe, pose, None, model, want=("qpos",))
    K.assert_near_lock_row(q[0], rv)
    zyx = np.zeros(3)
    probe.uhc_smpl_probe_euler(np.ascontiguousarray(rv).ctypes.data_as(C.c_void_p), zyx.ctypes.data_as(C.c_void_p))
    assert np.array_equal(np.tile(zyx, 23), q[0, 7:])  # the single-joint entry is the row's arithmetic


def test_probe_matches_the_values_recorded_from_the_reference(probe, model):
    from uhc_amd.model.mjcf import ball_variant
    g2 = np.load(os.path.join(G, "g2_smpl_to_qpose_standing.npz"))
    np.testing.assert_allclose(probe_rows(probe, g2["pose_aa"], None, model, want=("qpos",))[0], g2["qpos"], atol=2e-6, rtol=0)
    g3 = np.load(os.path.join(G, "g3_qpos_fk.npz"))
    np.testing.assert_allclose(probe_rows(probe, g3["pose_aa"], g3["trans"], model, want=("qpos",))[0], g3["f_qpos"], atol=2e-6, rtol=0)
    g14 = np.load(os.path.join(G, "g14_ball_env.npz"))
    np.testing.assert_allclose(probe_rows(probe, g14["pose_aa"], g14["trans"], ball_variant(model), want=("qpos_quat",))[1], g14["qpos_quat"], atol=2e-6, rtol=0)


# ---------------------------------------------------------------- 2. the surface
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from uhc_amd import _lib
    return _lib.lib()


ARGS = ["stream", "n_joint", "h_smpl_to_model", "d_root_offset", "n_models", "d_pose_aa", "d_trans", "n_frames", "d_clip_start", "d_clip_model", "n_clips", "d_qpos",
        "d_qpos_quat"]


def _table():
    from uhc_amd.sim import load_asset_model
    return np.ascontiguousarray(K.slot_of_joint(load_asset_model())[0], dtype=np.int32)


def _call(L, **over):
    a = dict(stream=None, n_joint=24, h_smpl_to_model=_table(), d_root_offset=FAKE, n_models=1, d_pose_aa=FAKE, d_trans=FAKE, n_frames=0, d_clip_start=FAKE,
             d_clip_model=None, n_clips=1, d_qpos=FAKE, d_qpos_quat=FAKE)
    a.update(over)
    a["h_smpl_to_model"] = None if a["h_smpl_to_model"] is None else a["h_smpl_to_model"].ctypes.data_as(C.POINTER(C.c_int32))
    rc = L.uhc_smpl_qpos(*[a[k] for k in ARGS])
    return rc, L.uhc_last_error().decode()


def test_header_declares_it_and_the_abi_is_still_11(L):
    from uhc_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uhc_amd.h")).read(), flags=re.S)
    assert re.search(r"\buhc_smpl_qpos\s*\(", header)
    assert "uhc_smpl_qpos" in _lib.SYMBOLS and hasattr(L, "uhc_smpl_qpos")
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T uhc_smpl_qpos$", dyn, flags=re.M)
    assert int(re.search(r"#define UHC_ABI_VERSION (\d+)", header).group(1)) == 11
    assert L.uhc_abi_version() == 11
    # the declared parameter list is the one this file calls with
    decl = re.search(r"\buhc_smpl_qpos\s*\((.*?)\);", header, flags=re.S).group(1)
    assert [re.search(r"(\w+)\s*$", p).group(1) for p in decl.split(",")] == ARGS


def test_an_empty_call_succeeds_without_a_launch(L):
    assert _call(L)[0] == 0
    # what may be absent: the translation, the root offset (count_offset=False), the clips' models, one of the two outputs
    assert _call(L, d_trans=None, d_root_offset=None, d_clip_model=None)[0] == 0
    assert _call(L, d_qpos=None)[0] == 0 and _call(L, d_qpos_quat=None)[0] == 0
    assert _call(L, d_clip_model=FAKE, n_models=3, n_clips=5)[0] == 0


@pytest.mark.parametrize("over,name", [
    (dict(n_joint=23), "n_joint"), (dict(n_joint=25), "n_joint"), (dict(n_joint=52), "n_joint"),
    (dict(h_smpl_to_model=None), "h_smpl_to_model"), (dict(d_pose_aa=None), "d_pose_aa"), (dict(d_clip_start=None), "d_clip_start"),
    (dict(d_qpos=None, d_qpos_quat=None), "d_qpos_quat"), (dict(d_qpos=None, d_qpos_quat=None), "d_qpos "),
    (dict(n_frames=-1), "n_frames"), (dict(n_clips=0), "n_clips"), (dict(n_clips=-2), "n_clips"), (dict(n_models=0), "n_models"), (dict(n_models=-1), "n_models"),
    (dict(d_qpos=C.c_void_p(0x1008)), "d_qpos "), (dict(d_qpos_quat=C.c_void_p(0x1008)), "d_qpos_quat"),
])
def test_bad_arguments_are_refused_by_name(L, over, name):
    # (n_frames stays 0 where the case does not set it: the checks come before the empty return, and a call that slipped through one would return 0 and fail
    #  here without ever launching on the fake pointers)
    rc, msg = _call(L, **over)
    assert rc != 0 and "uhc_smpl_qpos" in msg and name in msg, (rc, msg)


def test_a_table_that_is_no_permutation_is_refused_with_its_index(L):
    t = _table()
    assert sorted(t) == list(range(24)) and t[0] == 0  # the asset's own table passes the rule
    # (entry changed, its new value, the entry the refusal names: a duplicate is met at its SECOND occurrence)
    for m, j, named in [(0, 1, 0), (1, 0, 1), (5, 24, 5), (5, -1, 5), (7, int(t[3]), 7), (3, int(t[7]), 7), (23, int(t[22]), 23), (23, 1000, 23)]:
        bad = t.copy()
        bad[m] = j
        rc, msg = _call(L, h_smpl_to_model=bad)
        assert rc != 0 and "uhc_smpl_qpos" in msg and f"h_smpl_to_model[{named}]" in msg, (m, j, rc, msg)


def test_config_converts_on_the_host_by_default_and_refuses_an_unknown_value(tmp_path):
    import yaml
    from uhc_amd.utils.config_utils.copycat_config import Config
    assert Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path)).bank_convert == "host"
    shipped = yaml.safe_load(open(os.path.join(ROOT, "config", "uhc_amd", "copycat_mi355x.yml")))
    for value in ("device", "host"):
        assert Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path), cfg_dict=dict(shipped, bank_convert=value)).bank_convert == value
    with pytest.raises(ValueError, match="bogus"):
        Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path), cfg_dict=dict(shipped, bank_convert="bogus"))


def test_the_convert_switch_is_checked_before_anything_touches_a_device():
    from uhc_amd.envs.humanoid_im import VecHumanoidEnv
    env = object.__new__(VecHumanoidEnv)  # (the checks come before anything the method reads: no device needed)
    with pytest.raises(ValueError, match="bogus"):
        env.set_clip_bank({}, build="device", convert="bogus")
    with pytest.raises(ValueError, match="build='device'"):
        env.set_clip_bank({}, build="host", convert="device")
    for f in (VecHumanoidEnv.set_clip_bank, VecHumanoidEnv.set_clip_bank_from_loader):
        assert inspect.signature(f).parameters["convert"].default == "host"
        assert inspect.signature(f).parameters["build"].default == "host"


def test_the_single_clip_entry_refuses_what_the_host_function_refuses(model):
    from uhc_amd.smpllib.smpl_mujoco import smpl_to_qpose, smpl_to_qpose_device
    pose = np.zeros((2, 72))
    for kw in (dict(normalize=True), dict(random_root=True), dict(model="smplh")):
        with pytest.raises(NotImplementedError) as host:
            smpl_to_qpose(pose, model, **kw)
        with pytest.raises(NotImplementedError) as dev:
            smpl_to_qpose_device(pose, model, **kw)
        assert str(dev.value) == str(host.value)
    a, b = inspect.signature(smpl_to_qpose).parameters, inspect.signature(smpl_to_qpose_device).parameters
    assert list(a) == list(b) and all(a[k].default == b[k].default for k in a)
