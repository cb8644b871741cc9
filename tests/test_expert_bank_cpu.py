"""CPU: the C-ABI surface of uhc_expert_frames (the clip bank's frame records computed on the device) -- declaration, export, ABI version, and every
argument check, which the library makes BEFORE its first HIP call (so none of this needs a GPU) -- and the Python switches around it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)  # a non-null "device pointer": every call here has n_frames <= 0: refused or empty, nothing is launched and nothing dereferences it


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from uhc_amd import _lib
    return _lib.lib()


def _parents():
    from uhc_amd.sim import load_asset_model
    from uhc_amd.smpllib.torch_smpl_humanoid import Humanoid
    h = Humanoid(model=load_asset_model())
    return np.ascontiguousarray(h._parents, dtype=np.int32), np.ascontiguousarray(h._ee_idx, dtype=np.int32)


def _call(L, **over):
    par, ee = _parents()
    a = dict(stream=None, n_body=24, h_parent=par, h_ee_body=ee, d_body_pos=FAKE, d_body_ipos=FAKE, n_models=1, d_qpos=FAKE, n_frames=0,
             d_clip_start=FAKE, d_clip_model=None, n_clips=1, d_root_quat_record=None, dt=1 / 30, d_frames=FAKE)
    a.update(over)
    hp = None if a["h_parent"] is None else a["h_parent"].ctypes.data_as(C.POINTER(C.c_int32))
    he = None if a["h_ee_body"] is None else a["h_ee_body"].ctypes.data_as(C.POINTER(C.c_int32))
    rc = L.uhc_expert_frames(a["stream"], a["n_body"], hp, he, a["d_body_pos"], a["d_body_ipos"], a["n_models"], a["d_qpos"], a["n_frames"],
                             a["d_clip_start"], a["d_clip_model"], a["n_clips"], a["d_root_quat_record"], a["dt"], a["d_frames"])
    return rc, L.uhc_last_error().decode()


def test_header_declares_it_and_the_abi_is_11(L):
    from uhc_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uhc_amd.h")).read(), flags=re.S)
    assert re.search(r"\buhc_expert_frames\s*\(", header)
    assert "uhc_expert_frames" in _lib.SYMBOLS
    assert int(re.search(r"#define UHC_ABI_VERSION (\d+)", header).group(1)) == 11
    assert L.uhc_abi_version() == 11


def test_an_empty_bank_succeeds_without_a_launch(L):
    rc, _ = _call(L, n_frames=0)
    assert rc == 0


@pytest.mark.parametrize("over,names", [
    (dict(n_body=23), "n_body"), (dict(n_body=25), "n_body"),
    (dict(h_parent=None), "h_parent"), (dict(h_ee_body=None), "h_ee_body"), (dict(d_body_pos=None), "d_body_pos"),
    (dict(d_body_ipos=None), "d_body_ipos"), (dict(d_qpos=None), "d_qpos"), (dict(d_clip_start=None), "d_clip_start"),
    (dict(d_frames=None), "d_frames"),
    (dict(n_frames=-1), "n_frames"), (dict(n_clips=0), "n_clips"), (dict(n_clips=-3), "n_clips"), (dict(n_models=0), "n_models"),
    (dict(dt=0.0), "dt"), (dict(dt=-1 / 30), "dt"), (dict(dt=float("nan")), "dt"),
])
def test_bad_arguments_are_refused_by_name(L, over, names):
    # (n_frames stays 0 where the case does not set it: the checks come before the empty-bank return, and a call that slipped through one would
    #  return 0 and fail here without ever launching on the fake pointers)
    rc, msg = _call(L, **over)
    assert rc != 0 and "uhc_expert_frames" in msg and names in msg, (rc, msg)


def test_a_parent_that_does_not_precede_its_child_is_refused(L):
    par, _ = _parents()
    assert par[0] == -1 and all(0 <= par[i] < i for i in range(1, 24))  # the asset's own tree passes the rule
    for i, p in [(0, 0), (1, -1), (5, 5), (5, 7), (23, 24), (3, -2)]:
        bad = par.copy()
        bad[i] = p
        rc, msg = _call(L, h_parent=bad)
        assert rc != 0 and f"h_parent[{i}]" in msg, (i, p, rc, msg)


def test_an_end_effector_outside_the_bodies_is_refused(L):
    _, ee = _parents()
    for k, v in [(0, -1), (4, 24), (2, 1000)]:
        bad = ee.copy()
        bad[k] = v
        rc, msg = _call(L, h_ee_body=bad)
        assert rc != 0 and f"h_ee_body[{k}]" in msg, (k, v, rc, msg)


def test_config_builds_the_bank_on_the_host_by_default(tmp_path):
    from uhc_amd.utils.config_utils.copycat_config import Config
    assert Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path)).bank_build == "host"


def test_an_unknown_build_is_a_value_error():
    from uhc_amd.envs.humanoid_im import VecHumanoidEnv
    env = object.__new__(VecHumanoidEnv)  # (the check comes before anything the method reads: no device needed)
    with pytest.raises(ValueError, match="bogus"):
        env.set_clip_bank({}, build="bogus")
    import inspect
    assert inspect.signature(VecHumanoidEnv.set_clip_bank).parameters["build"].default == "host"
    assert inspect.signature(VecHumanoidEnv.set_clip_bank_from_loader).parameters["build"].default == "host"
