"""CPU: the evaluation kernels' arithmetic and surface without a GPU.  (1) uhc_amd/csrc/uhc_eval_metrics.h -- the per-row arithmetic uhc_eval.hip computes with,
lane = joint -- compiled for the host (tests/eval_metrics_probe.cpp, its sums over the joints as plain loops) against the values the reference recorded and
against compute_metrics; (2) the C-ABI surface of uhc_eval_record / uhc_eval_metrics: declaration, export, ABI version and every argument check, which the library
makes BEFORE its first HIP call; the config key."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import probe_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["root_dist", "vel_dist", "accel_dist", "mpjpe_g", "pa_mpjpe", "mpjpe"]  # a row of the kernels' output, in order
SENTINEL = -7.0
FAKE = C.c_void_p(0x1000)  # a non-null "device pointer": every call here is refused or has n_env == 0 -- nothing is launched and nothing dereferences it


def build_probe():
    """tests/eval_metrics_probe.cpp + uhc_eval_metrics.h -> uhc_amd/csrc/build/eval_metrics_probe.so with the host compiler: no hipcc, no HIP header."""
    return probe_build.build_probe("eval_metrics_probe.so", ["tests/eval_metrics_probe.cpp"], ["uhc_amd/csrc/uhc_eval_metrics.h"], probe_build.NO_CONTRACT)


@pytest.fixture(scope="module")
def probe():
    return C.CDLL(build_probe())


def probe_clip(P, pred, gt, pj, gj):
    """-> [T][6], SENTINEL where the probe wrote nothing"""
    a = [np.ascontiguousarray(x, dtype=np.float64) for x in (pred, gt, pj, gj)]
    T = a[0].shape[0]
    assert a[1].shape[0] == T and a[2].shape == a[3].shape == (T, 72)
    out = np.full((T, 6), SENTINEL)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    P.uhc_eval_probe_clip(p(a[0]), C.c_int(a[0].shape[1]), p(a[1]), C.c_int(a[1].shape[1]), p(a[2]), p(a[3]), C.c_int(T), p(out))
    return out


def assert_clip_matches(out, ref, atol=1e-9):
    """the six columns against compute_metrics' arrays: numpy's lengths (T, T - 1, T - 2), nothing written beyond them"""
    for k, name in enumerate(NAMES):
        n = len(ref[name])
        np.testing.assert_allclose(out[:n, k], ref[name], atol=atol, rtol=0, err_msg=name)
        assert (out[n:, k] == SENTINEL).all(), name


def random_clip(rng, T, noise=0.1, nqh=76):
    gj = rng.normal(size=(T, 24, 3))
    pj = gj + noise * rng.normal(size=gj.shape)
    pq, gq = rng.normal(size=(T, nqh)), rng.normal(size=(T, 76))  # (root quaternions of any length: quaternion_matrix normalises)
    return pq, gq, pj.reshape(T, 72), gj.reshape(T, 72)


def reference(pq, gq, pj, gj):
    from uhc_amd.smpllib.smpl_eval import compute_metrics
    return compute_metrics(dict(pred=pq, gt=gq, pred_jpos=pj, gt_jpos=gj, fail_safe=False, percent=1))


# ---------------------------------------------------------------- 1. the arithmetic
def test_probe_matches_the_values_recorded_from_the_reference(probe):
    g = np.load(os.path.join(ROOT, "tests", "golden", "g11_metrics.npz"))
    out = probe_clip(probe, g["pred"], g["gt"], g["pred_jpos"], g["gt_jpos"])
    assert out.shape == (30, 6)
    assert_clip_matches(out, {n: g["m_" + n] for n in NAMES})  # atol 1e-9: the bar tests/test_reference_golden.py sets for the numpy version


def test_probe_matches_compute_metrics_on_random_poses(probe):
    rng = np.random.default_rng(11)
    for T, nqh in ((12, 76), (7, 99)):
        c = random_clip(rng, T, nqh=nqh)
        assert_clip_matches(probe_clip(probe, *c), reference(*c))


def test_probe_matches_when_pred_is_gt_plus_rounding_noise(probe):
    # H is then symmetric to 1e-13: off-diagonal elements of H^T H that Jacobi has to skip, not rotate by an overflowing angle
    rng = np.random.default_rng(12)
    c = random_clip(rng, 10, noise=1e-13)
    out = probe_clip(probe, *c)
    assert np.isfinite(out[:, 4]).all()
    assert_clip_matches(out, reference(*c))


def test_probe_matches_on_a_mirrored_pred(probe):
    # det(V U^T) < 0: p_mpjpe's determinant branch flips V's last column and the last singular value
    rng = np.random.default_rng(13)
    pq, gq, pj, gj = random_clip(rng, 9)
    pj = (gj.reshape(-1, 24, 3) * np.array([1.0, 1.0, -1.0]) + 0.01 * rng.normal(size=(9, 24, 3))).reshape(9, 72)
    ref = reference(pq, gq, pj, gj)
    assert ref["pa_mpjpe"].min() > 10.0  # (a reflection cannot be rotated away)
    assert_clip_matches(probe_clip(probe, pq, gq, pj, gj), ref)


@pytest.mark.parametrize("T", [2, 3])
def test_probe_matches_on_the_shortest_clips(probe, T):
    rng = np.random.default_rng(20 + T)
    c = random_clip(rng, T)
    ref = reference(*c)
    assert len(ref["vel_dist"]) == T - 1 and len(ref["accel_dist"]) == T - 2
    assert_clip_matches(probe_clip(probe, *c), ref)


def test_svd3_reproduces_its_matrix_also_where_it_is_rank_deficient(probe):
    rng = np.random.default_rng(14)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    planar = rng.normal(size=(3, 3))
    planar[:, 2] = 0.0  # a cloud in a plane: the third singular value vanishes, u_2 comes from the cross product
    for H in (rng.normal(size=(3, 3)), np.diag([3.0, 2.0, 1.0]), np.eye(3) + 1e-13 * rng.normal(size=(3, 3)), planar):
        H = np.ascontiguousarray(H)
        U, s, V = np.zeros((3, 3)), np.zeros(3), np.zeros((3, 3))
        probe.uhc_eval_probe_svd3(p(H), p(U), p(s), p(V))
        assert np.isfinite(U).all() and np.isfinite(V).all()
        np.testing.assert_allclose(s, np.linalg.svd(H, compute_uv=False), atol=1e-14)
        np.testing.assert_allclose(U @ np.diag(s) @ V.T, H, atol=1e-14)
        np.testing.assert_allclose(U.T @ U, np.eye(3), atol=1e-13)
        np.testing.assert_allclose(V.T @ V, np.eye(3), atol=1e-13)


# ---------------------------------------------------------------- 2. the surface
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from uhc_amd import _lib
    return _lib.lib()


RECORD_ARGS = ["stream", "phase", "n_env", "n_body", "nq", "nqh", "nbody", "row_cap", "t", "fail_safe", "d_qpos", "d_xpos", "d_clip0", "d_len", "d_done", "d_reward",
               "d_percent_in", "d_alive", "d_rows", "d_steps", "d_pred_qpos", "d_pred_jpos", "d_gt_frame", "d_rewards", "d_fail_safe", "d_percent", "d_tele", "d_overflow"]
METRICS_ARGS = ["stream", "n_env", "n_body", "nqh", "row_cap", "d_rows", "d_pred_qpos", "d_pred_jpos", "d_gt_frame", "d_frames", "n_frames", "d_row_metrics",
                "d_clip_means", "d_bad", "h_bad"]


def _record(L, **over):
    a = {k: FAKE for k in RECORD_ARGS if k.startswith("d_")}
    a.update(stream=None, phase=1, n_env=0, n_body=24, nq=76, nqh=76, nbody=25, row_cap=8, t=0, fail_safe=1)
    a.update(over)
    rc = L.uhc_eval_record(*[a[k] for k in RECORD_ARGS])
    return rc, L.uhc_last_error().decode()


def _metrics(L, **over):
    a = {k: FAKE for k in METRICS_ARGS if k.startswith("d_")}
    a.update(stream=None, n_env=0, n_body=24, nqh=76, row_cap=8, n_frames=10, h_bad=None)
    a.update(over)
    rc = L.uhc_eval_metrics(*[a[k] for k in METRICS_ARGS])
    return rc, L.uhc_last_error().decode()


def test_header_declares_both_and_the_abi_is_still_11(L):
    from uhc_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uhc_amd.h")).read(), flags=re.S)
    for name in ("uhc_eval_record", "uhc_eval_metrics"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert int(re.search(r"#define UHC_ABI_VERSION (\d+)", header).group(1)) == 11
    assert L.uhc_abi_version() == 11
    # the declared parameter lists are the ones this file calls with
    for name, args in (("uhc_eval_record", RECORD_ARGS), ("uhc_eval_metrics", METRICS_ARGS)):
        decl = re.search(r"\b" + name + r"\s*\((.*?)\);", header, flags=re.S).group(1)
        assert [re.search(r"(\w+)\s*$", p).group(1) for p in decl.split(",")] == args


def test_no_envs_succeed_without_a_launch(L):
    assert _record(L)[0] == 0 and _record(L, phase=0, d_done=None, d_reward=None, d_percent_in=None)[0] == 0
    assert _metrics(L)[0] == 0
    h = C.c_int32(5)
    assert _metrics(L, h_bad=C.byref(h))[0] == 0 and h.value == 0


@pytest.mark.parametrize("over,name", [(dict(n_body=23), "n_body"), (dict(n_body=25), "n_body"), (dict(row_cap=0), "row_cap"), (dict(row_cap=-4), "row_cap"),
                                       (dict(n_env=-1), "n_env"), (dict(nqh=6), "nqh"), (dict(nqh=77), "nqh"), (dict(nq=113, nqh=114), "nqh"),
                                       (dict(nbody=24), "nbody"), (dict(phase=2), "phase"), (dict(phase=-1), "phase"), (dict(t=-1), "t")] +
                         [({k: None}, k) for k in RECORD_ARGS if k.startswith("d_")])
def test_record_refuses_bad_arguments_by_name(L, over, name):
    # (n_env stays 0: the checks come before the empty return, and a call that slipped through one would return 0 and fail here without launching)
    rc, msg = _record(L, **over)
    assert rc != 0 and "uhc_eval_record" in msg and name in msg, (rc, msg)


def test_record_takes_no_step_outputs_in_phase_0(L):
    assert _record(L, phase=0, d_done=None, d_reward=None, d_percent_in=None)[0] == 0
    assert _record(L, nq=113, nqh=99, nbody=27)[0] == 0  # ball joints plus two objects


@pytest.mark.parametrize("over,name", [(dict(n_body=23), "n_body"), (dict(row_cap=0), "row_cap"), (dict(n_env=-1), "n_env"), (dict(nqh=6), "nqh"),
                                       (dict(n_frames=-1), "n_frames")] +
                         [({k: None}, k) for k in METRICS_ARGS if k.startswith("d_")])
def test_metrics_refuses_bad_arguments_by_name(L, over, name):
    rc, msg = _metrics(L, **over)
    assert rc != 0 and "uhc_eval_metrics" in msg and name in msg, (rc, msg)


def test_config_evaluates_on_the_host_by_default_and_refuses_an_unknown_value(tmp_path):
    import yaml
    from uhc_amd.utils.config_utils.copycat_config import Config
    assert Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path)).eval_build == "host"
    shipped = yaml.safe_load(open(os.path.join(ROOT, "config", "uhc_amd", "copycat_mi355x.yml")))
    for value in ("device", "host"):
        assert Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path), cfg_dict=dict(shipped, eval_build=value)).eval_build == value
    with pytest.raises(ValueError, match="bogus"):
        Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path), cfg_dict=dict(shipped, eval_build="bogus"))
