"""CPU: the C-ABI surface of the live targets (uhc_env_live_begin / push / view / end: each env imitates a stream of frames appended while it runs) --
declaration, export, ABI version, and the argument checks.  The checks that do not read the env come first and `e == NULL` is the last one before any
HIP call, so with e = NULL every one of them is reached without a GPU: a bad argument is refused by ITS name, valid arguments are refused naming the env."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)  # a non-null "device pointer": every call here is refused or empty; nothing is launched and nothing dereferences it
NAMES = ["uhc_env_live_begin", "uhc_env_live_push", "uhc_env_live_view", "uhc_env_live_end"]


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


def _begin(L, **over):
    par, ee = _parents()
    a = dict(e=None, cap=8, n_body=24, h_parent=par, h_ee_body=ee, d_body_pos=FAKE, d_body_ipos=FAKE, n_models=1, dt=1 / 30, d_beta=None)
    a.update(over)
    hp = None if a["h_parent"] is None else a["h_parent"].ctypes.data_as(C.POINTER(C.c_int32))
    he = None if a["h_ee_body"] is None else a["h_ee_body"].ctypes.data_as(C.POINTER(C.c_int32))
    rc = L.uhc_env_live_begin(a["e"], a["cap"], a["n_body"], hp, he, a["d_body_pos"], a["d_body_ipos"], a["n_models"], a["dt"], a["d_beta"])
    return rc, L.uhc_last_error().decode()


def _push(L, **over):
    a = dict(e=None, d_env_ids=FAKE, n=1, d_qpos=FAKE, d_root_quat_record=None, d_restart=None, d_model=None)
    a.update(over)
    rc = L.uhc_env_live_push(a["e"], a["d_env_ids"], a["n"], a["d_qpos"], a["d_root_quat_record"], a["d_restart"], a["d_model"])
    return rc, L.uhc_last_error().decode()


def test_header_declares_them_and_the_abi_is_11(L):
    from uhc_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uhc_amd.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert int(re.search(r"#define UHC_ABI_VERSION (\d+)", header).group(1)) == 11
    assert L.uhc_abi_version() == 11


@pytest.mark.parametrize("over,names", [
    (dict(cap=1), "cap"), (dict(cap=0), "cap"), (dict(cap=-1), "cap"),
    (dict(n_body=23), "n_body"), (dict(n_body=25), "n_body"),
    (dict(h_parent=None), "h_parent"), (dict(h_ee_body=None), "h_ee_body"), (dict(d_body_pos=None), "d_body_pos"), (dict(d_body_ipos=None), "d_body_ipos"),
    (dict(dt=0.0), "dt"), (dict(dt=-1 / 30), "dt"), (dict(dt=float("nan")), "dt"),
    (dict(n_models=0), "n_models"),
])
def test_live_begin_refuses_bad_arguments_by_name(L, over, names):
    rc, msg = _begin(L, **over)
    assert rc != 0 and "uhc_env_live_begin" in msg and names in msg and "the env e" not in msg, (rc, msg)


def test_live_begin_refuses_a_parent_that_does_not_precede_its_child(L):
    par, _ = _parents()
    assert par[0] == -1 and all(0 <= par[i] < i for i in range(1, 24))  # the asset's own tree passes the rule
    for i, p in [(0, 0), (1, -1), (5, 5), (5, 7), (23, 24), (3, -2)]:
        bad = par.copy()
        bad[i] = p
        rc, msg = _begin(L, h_parent=bad)
        assert rc != 0 and "uhc_env_live_begin" in msg and f"h_parent[{i}]" in msg, (i, p, rc, msg)


def test_live_begin_refuses_an_end_effector_outside_the_bodies(L):
    _, ee = _parents()
    for k, v in [(0, -1), (4, 24), (2, 1000)]:
        bad = ee.copy()
        bad[k] = v
        rc, msg = _begin(L, h_ee_body=bad)
        assert rc != 0 and "uhc_env_live_begin" in msg and f"h_ee_body[{k}]" in msg, (k, v, rc, msg)


@pytest.mark.parametrize("over,names", [(dict(d_env_ids=None), "d_env_ids"), (dict(d_qpos=None), "d_qpos"), (dict(n=-1), "n < 0")])
def test_live_push_refuses_bad_arguments_by_name(L, over, names):
    rc, msg = _push(L, **over)
    assert rc != 0 and "uhc_env_live_push" in msg and names in msg and "the env e" not in msg, (rc, msg)


def test_valid_arguments_are_refused_naming_the_env(L):
    rc, msg = _begin(L)
    assert rc != 0 and "uhc_env_live_begin" in msg and "the env e is NULL" in msg, (rc, msg)
    rc, msg = _push(L)
    assert rc != 0 and "uhc_env_live_push" in msg and "the env e is NULL" in msg, (rc, msg)
    assert L.uhc_env_live_end(None) != 0 and "uhc_env_live_end" in L.uhc_last_error().decode()
    assert L.uhc_env_live_view(None, None, None, None, None) != 0 and "uhc_env_live_view" in L.uhc_last_error().decode()


def test_an_empty_push_succeeds_without_a_launch(L):
    rc, _ = _push(L, n=0)  # (nothing to push: nothing of the env is read, nothing is launched on the fake pointers)
    assert rc == 0


def test_python_surface_exists():
    import inspect
    from uhc_amd.envs.humanoid_im import VecHumanoidEnv
    from uhc_amd.sim import EnvBatch
    from uhc_amd.stream import StreamTracker
    for cls, names in ((EnvBatch, ("live_begin", "live_push", "live_view", "live_end")),
                       (VecHumanoidEnv, ("live_begin", "live_push", "live_push_smpl", "live_end")), (StreamTracker, ("begin", "step"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    assert list(inspect.signature(EnvBatch.live_push).parameters)[1:] == ["env_ids", "qpos", "restart", "root_quat_record", "model"]
    assert inspect.signature(EnvBatch.live_begin).parameters["dt"].default == 1 / 30
