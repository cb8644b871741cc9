"""CPU: the C-ABI and Python surface of the sliding live window (uhc_env_live_slide / uhc_env_live_window: a stream of any length in a bank of `cap` frames) --
declaration, export, ABI version, the refusal with e = NULL, the Python signatures, and track_stream's check of `cap`, which comes before anything
touches a device."""
import ctypes as C
import inspect
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uhc_env_live_slide", "uhc_env_live_window"]


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from uhc_amd import _lib
    return _lib.lib()


def test_header_declares_them_and_the_abi_stays_11(L):
    from uhc_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uhc_amd.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert int(re.search(r"#define UHC_ABI_VERSION (\d+)", header).group(1)) == 11
    assert L.uhc_abi_version() == 11


def test_without_an_env_each_call_is_refused_naming_the_env(L):
    for on in (0, 1):
        assert L.uhc_env_live_slide(None, on) != 0
        msg = L.uhc_last_error().decode()
        assert "uhc_env_live_slide" in msg and "the env e is NULL" in msg, msg
    base, moved = C.c_void_p(), C.c_void_p()
    for args in ((None, None), (C.byref(base), C.byref(moved))):
        assert L.uhc_env_live_window(None, *args) != 0
        msg = L.uhc_last_error().decode()
        assert "uhc_env_live_window" in msg and "the env e is NULL" in msg, msg
    assert base.value is None and moved.value is None  # (nothing was written)


def test_python_surface_exists():
    from uhc_amd.agents.agent_copycat import AgentCopycat
    from uhc_amd.envs.humanoid_im import VecHumanoidEnv
    from uhc_amd.sim import EnvBatch
    sig = inspect.signature
    assert list(sig(EnvBatch.live_slide).parameters) == ["self", "on"] and sig(EnvBatch.live_slide).parameters["on"].default is True
    assert list(sig(EnvBatch.live_window).parameters) == ["self"]
    assert list(sig(VecHumanoidEnv.live_begin).parameters) == ["self", "cap", "beta", "slide"]
    assert sig(VecHumanoidEnv.live_begin).parameters["beta"].default is None and sig(VecHumanoidEnv.live_begin).parameters["slide"].default is False
    assert list(sig(VecHumanoidEnv.live_window).parameters) == ["self"]
    p = sig(AgentCopycat.track_stream).parameters
    assert list(p) == ["self", "source", "n_steps", "n_env", "head", "cap"]
    assert p["n_env"].default is None and p["head"].default == 3 and p["cap"].default is None
    for fn in (VecHumanoidEnv.live_begin, EnvBatch.live_slide):
        assert "percent" in fn.__doc__.lower() and "window" in fn.__doc__.lower()
    assert "reset" in VecHumanoidEnv.live_begin.__doc__ and "oldest kept frame" in VecHumanoidEnv.live_begin.__doc__


@pytest.mark.parametrize("head,cap", [(3, 3), (3, 2), (2, 2), (5, 5), (3, 0)])
def test_track_stream_refuses_a_cap_below_head_plus_one_by_name(head, cap):
    from uhc_amd.agents.agent_copycat import AgentCopycat
    me = types.SimpleNamespace(cfg=types.SimpleNamespace(n_env=2))  # (the check comes before any env or device is touched)

    def source(t):
        raise AssertionError("the source must not be asked for a frame")

    with pytest.raises(ValueError, match="cap") as err:
        AgentCopycat.track_stream(me, source, 8, head=head, cap=cap)
    assert "track_stream" in str(err.value) and "dropped" in str(err.value) and f"head + 1 = {head + 1}" in str(err.value)
