"""CPU: the surface metrics (penetration, skate, float, contact count) without a GPU.  (1) uhc_amd/csrc/uhc_surface_math.h -- the per-vertex arithmetic
uhc_surface.hip computes with, the vertices dealt to the lanes -- compiled for the host (tests/surface_metrics_probe.cpp, its sums as plain loops) against
smpl_eval.compute_penetration / compute_skate / compute_float on hull_vertices, and both against the values recorded from the reference's own functions;
(2) the C-ABI surface of uhc_surface_create / uhc_surface_metrics / uhc_eval_record_pose: declaration, export, ABI version and every argument check, which the
library makes BEFORE its first HIP call; the config key."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import probe_build
from tests import surface_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)  # a non-null "device pointer": every call here is refused or has nothing to do -- nothing is launched and nothing dereferences it
ATOL = 1e-9  # mm


def build_probe():
    """tests/surface_metrics_probe.cpp + uhc_surface_math.h -> uhc_amd/csrc/build/surface_metrics_probe.so with the host compiler: no hipcc, no HIP header."""
    return probe_build.build_probe("surface_metrics_probe.so", ["tests/surface_metrics_probe.cpp"], ["uhc_amd/csrc/uhc_surface_math.h", "uhc_amd/csrc/uhc_seq.h"],
                                   probe_build.NO_CONTRACT)


@pytest.fixture(scope="module")
def probe():
    return C.CDLL(build_probe())


def _ptr(x):
    return x.ctypes.data_as(C.c_void_p) if x is not None else None


def probe_seq(P, vert, vert_body, vert_radius, pos, quat, floor_z):
    """-> (rows [T][4] with SENTINEL where the probe wrote nothing, means [4], bad)"""
    vert, pos, quat = (np.ascontiguousarray(a, dtype=np.float64) for a in (vert, pos, quat))
    vb = np.ascontiguousarray(vert_body, dtype=np.int32)
    vr = None if vert_radius is None else np.ascontiguousarray(vert_radius, dtype=np.float64)
    T, B = pos.shape[0], pos.shape[1]
    assert pos.shape == (T, B, 3) and quat.shape == (T, B, 4) and vert.shape == (len(vb), 3)
    rows, means = np.full((T, 4), SC.SENTINEL), np.full(4, SC.SENTINEL)
    bad = P.uhc_surface_probe_seq(C.c_int(B), C.c_int(len(vb)), _ptr(vb), _ptr(vr), _ptr(vert), _ptr(pos), _ptr(quat), C.c_int(T), C.c_double(floor_z), _ptr(rows),
                                  _ptr(means))
    return rows, means, bad


def probe_case(P, c, model=None):
    return probe_seq(P, c["vert"][c["model"] if model is None else model], c["vert_body"], c["vert_radius"], c["pos"], c["quat"], c["floor_z"])


# ---------------------------------------------------------------- 1. the arithmetic
@pytest.mark.parametrize("kind", SC.KINDS)
def test_probe_matches_the_host_functions(probe, kind):
    for V in SC.VERTS:
        for T in SC.ROWS:
            c = SC.make_case(kind, V, T)
            rows, means, bad = probe_case(probe, c)
            exp_rows, exp_means, exp_bad = SC.expected(c)
            SC.assert_rows_match(rows, means, exp_rows, exp_means, (kind, V, T), atol=ATOL)
            assert bad == exp_bad, (kind, V, T)
            if T == 1:
                assert np.isnan(means[1]) and rows[0, 1] == SC.SENTINEL  # no pair of rows: the mean over nothing


def test_the_cases_are_what_their_names_say(probe):
    for V in SC.VERTS:
        rows, _, _ = SC.expected(SC.make_case("clear", V, 5))
        assert (rows[:, 0] == 0).all() and (rows[:4, 1] == 0).all() and (rows[:, 2] > 0).all() and (rows[:, 3] == 0).all()
        rows, _, _ = SC.expected(SC.make_case("sunk", V, 5))
        assert (rows[:, 0] > 0).all() and (rows[:4, 1] > 0).all() and (rows[:, 2] == 0).all() and (rows[:, 3] == V).all()
        c = SC.make_case("radius", V, 5)
        assert not np.array_equal(SC.expected(c)[0], SC.expected(dict(c, vert_radius=None))[0])  # the radius lowers every vertex
        c = SC.make_case("floor", V, 5)
        assert not np.array_equal(SC.expected(c)[0], SC.expected(dict(c, floor_z=0.0))[0])
        c = SC.make_case("models", V, 5)
        assert c["model"] == 1 and not np.array_equal(probe_case(probe, c)[0], probe_case(probe, c, model=0)[0])
    seen = [SC.expected(SC.make_case("mixed", 130, 5))[0]]
    assert ((seen[0][:, 0] > 0) & (seen[0][:, 3] > 0) & (seen[0][:, 3] < 130)).any()  # some vertices below, some above, in one row


@pytest.mark.parametrize("V", SC.VERTS)
def test_a_vertex_exactly_on_the_floor_counts_for_skate_and_contact_not_for_penetration(probe, V):
    c = SC.make_case("exact", V, 5)
    h = SC.heights(c)
    assert (h[:, 0] == 0.0).all()  # exactly, on the host ...
    out = np.zeros(7)
    for r in range(5):  # ... and in the header's arithmetic
        p, q, v = (np.ascontiguousarray(a, dtype=np.float64) for a in (c["pos"][r, 0], c["quat"][r, 0], c["vert"][0, 0]))
        probe.uhc_surface_probe_vertex(_ptr(p), _ptr(q), _ptr(v), C.c_double(0.0), C.c_double(0.0), _ptr(out))
        assert out[3] == 0.0 and list(out[4:]) == [0.0, 1.0, 0.0], out
    rows, means, bad = probe_case(probe, c)
    exp_rows, exp_means, _ = SC.expected(c)
    SC.assert_rows_match(rows, means, exp_rows, exp_means, ("exact", V))
    # with the vertex taken out, every row has one contact less, and the same penetration: it never counted as below the floor
    if V > 1:
        less = dict(c, V=V - 1, vert=c["vert"][:, 1:], vert_body=c["vert_body"][1:])
        rows1, _, _ = probe_case(probe, less)
        np.testing.assert_array_equal(rows1[:, 3], rows[:, 3] - 1)
        np.testing.assert_array_equal(rows1[:, 0], rows[:, 0])
    else:
        assert (rows[:, 0] == 0).all() and (rows[:, 3] == 1).all() and (rows[:, 2] == 0).all()
        from uhc_amd.smpllib.smpl_eval import hull_vertices
        w = hull_vertices(SC.tables(c), c["pos"], c["quat"])  # the one vertex touches the floor in every row: its skate is how far it slides
        np.testing.assert_allclose(rows[:4, 1], np.linalg.norm(w[1:, 0, :2] - w[:-1, 0, :2], axis=1) * 1000, atol=ATOL, rtol=0)


@pytest.mark.parametrize("has_next", [False, True])
@pytest.mark.parametrize("row_ok,next_ok", [(True, True), (True, False), (False, True), (False, False)])
def test_store_row_writes_nan_for_a_bad_row_and_leaves_the_skate_of_a_last_row_alone(probe, has_next, row_ok, next_ok):
    # uhc_sf_store_row is the function uhc_surface_rows_kernel, uhc_smpl_mesh_kernel and the host loop all finish a row with
    V = 7
    for acc in ([-0.06, 0.012, -0.03, 3, 2, 4, 3], [0.0, 0.0, 0.25, 0, 0, 0, V]):  # some vertices below the floor and sliding; every vertex above it
        out = np.full(4, SC.SENTINEL)
        probe.uhc_surface_probe_store_row(_ptr(np.array(acc, dtype=np.float64)), C.c_int(V), C.c_int(has_next), C.c_int(row_ok), C.c_int(next_ok), _ptr(out))
        pen_sum, skate_sum, h_min, pen_n, skate_n, contact_n, above_n = acc
        want = [-(pen_sum / pen_n) * 1000.0 if pen_n else 0.0, skate_sum / skate_n * 1000.0 if skate_n else 0.0, h_min * 1000.0 if above_n == V else 0.0, float(contact_n)]
        if not row_ok:
            want = [np.nan] * 4
        elif not next_ok:
            want[1] = np.nan
        if not has_next:
            want[1] = SC.SENTINEL  # the slot is not touched: no row r + 1, no skate
        np.testing.assert_array_equal(out, want)  # (NaN equals NaN here; the finite values are the same expressions: exact)


def test_host_functions_and_probe_reproduce_the_values_recorded_from_the_reference(probe):
    from uhc_amd.smpllib import smpl_eval as E
    g = np.load(os.path.join(ROOT, "tests", "golden", "g17_surface.npz"))
    T, V = g["pos"].shape[0], g["vert"].shape[0]
    assert (T, V) == (20, 200) and g["pen"].shape == (T,) and g["skate"].shape == (T - 1,)
    info = {"floor_z": 0}
    world = E.hull_vertices((g["vert"], g["vert_body"], np.zeros(V)), g["pos"], g["quat"])  # (what the reference's functions were handed)
    np.testing.assert_allclose(E.compute_penetration(world, info), g["pen"], atol=ATOL, rtol=0)
    np.testing.assert_allclose(E.compute_skate(world, info), g["skate"], atol=ATOL, rtol=0)
    rows, means, bad = probe_seq(probe, g["vert"], g["vert_body"], None, g["pos"], g["quat"], 0.0)
    assert bad == 0
    np.testing.assert_allclose(rows[:, 0], g["pen"], atol=ATOL, rtol=0)
    np.testing.assert_allclose(rows[:T - 1, 1], g["skate"], atol=ATOL, rtol=0)
    np.testing.assert_allclose(means[:2], [g["pen"].mean(), g["skate"].mean()], atol=ATOL, rtol=0)
    # compute_metrics hands them on as the reference does: two scalars under its spelling, the vertices dropped
    rng = np.random.default_rng(17)
    res = dict(pred=rng.normal(size=(T, 76)), gt=rng.normal(size=(T, 76)), pred_jpos=rng.normal(size=(T, 72)), gt_jpos=rng.normal(size=(T, 72)), fail_safe=False,
               percent=1, pred_vertices=world)
    out = E.compute_metrics(res)
    assert "pred_vertices" not in res and np.ndim(out["pentration"]) == 0 and np.ndim(out["skate"]) == 0
    np.testing.assert_allclose([out["pentration"], out["skate"]], [g["pen"].mean(), g["skate"].mean()], atol=ATOL, rtol=0)
    assert out["contact"].shape == (T,) and np.ndim(out["float"]) == 0


def test_hull_vertices_of_the_asset_model_are_its_geoms_vertices():
    from uhc_amd.sim import load_asset_model
    from uhc_amd.smpllib import smpl_eval as E
    m = load_asset_model()
    vert, body, radius = E.surface_tables(m)
    assert vert.shape[0] == int(np.asarray(m.geom_vertnum)[np.asarray(m.geom_bodyid) >= 1].sum()) and body.min() == 0 and body.max() == 23 and (radius == 0).all()
    assert (np.bincount(body, minlength=24) > 3).all()  # every body part has a hull
    rng = np.random.default_rng(3)
    q = rng.normal(size=(2, 24, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    p = rng.normal(size=(2, 24, 3))
    w = E.hull_vertices(m, p, q)
    from uhc_amd.utils.transformation import quaternion_matrix
    for v in (0, 600, vert.shape[0] - 1):
        np.testing.assert_allclose(w[1, v], p[1, body[v]] + quaternion_matrix(q[1, body[v]])[:3, :3] @ vert[v], atol=1e-14)


# ---------------------------------------------------------------- 2. the surface
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from uhc_amd import _lib
    return _lib.lib()


CREATE_ARGS = ["n_body", "n_vert", "n_models", "h_vert_body", "h_vert_radius", "h_vert", "out"]
METRICS_ARGS = ["stream", "surf", "n_seq", "d_seq_start", "d_seq_rows", "row_cap", "d_seq_model", "d_pos", "pos_stride", "d_quat", "quat_stride", "n_rows_total",
                "floor_z", "d_row_out", "d_seq_means", "d_bad", "h_bad"]
POSE_ARGS = ["stream", "phase", "n_env", "nbody", "row_cap", "d_xpos", "d_xquat", "d_done", "d_alive", "d_rows", "d_pose"]


def _create(L, n_body=2, n_vert=3, n_models=1, body=(0, 1, 1), radius=(0.0, 0.1, 0.2), vert=None, out=True, null=()):
    vb = np.array(body, dtype=np.int32)
    vr = None if radius is None else np.array(radius, dtype=np.float64)
    vv = np.zeros((max(n_models, 1), len(vb), 3)) if vert is None else np.ascontiguousarray(vert, dtype=np.float64)
    h = C.c_void_p(0x1234)
    a = dict(n_body=n_body, n_vert=n_vert, n_models=n_models, h_vert_body=_ptr(vb), h_vert_radius=_ptr(vr), h_vert=_ptr(vv), out=C.byref(h) if out else None)
    for k in null:
        a[k] = None
    rc = L.uhc_surface_create(*[a[k] for k in CREATE_ARGS])
    return rc, L.uhc_last_error().decode(), h


@pytest.mark.parametrize("over,name", [(dict(n_body=0), "n_body"), (dict(n_body=65), "n_body"), (dict(n_vert=0), "n_vert"), (dict(n_vert=65536), "n_vert"),
                                       (dict(n_models=0), "n_models"), (dict(body=(0, 2, 1)), "h_vert_body"), (dict(body=(0, -1, 1)), "h_vert_body"),
                                       (dict(radius=(0.0, -0.1, 0.0)), "h_vert_radius"), (dict(radius=(0.0, np.nan, 0.0)), "h_vert_radius"),
                                       (dict(radius=(np.inf, 0.0, 0.0)), "h_vert_radius"),
                                       (dict(vert=[[[0, 0, 0], [0, np.nan, 0], [0, 0, 0]]]), "h_vert"), (dict(vert=[[[0, 0, 0], [0, 0, 0], [0, 0, -np.inf]]]), "h_vert"),
                                       (dict(null=("h_vert_body",)), "h_vert_body"), (dict(null=("h_vert",)), "h_vert"), (dict(out=False), "out")])
def test_create_refuses_bad_tables_by_name(L, over, name):
    # (every refusal comes before the first HIP call: this runs on a machine without a GPU)
    rc, msg, h = _create(L, **over)
    assert rc != 0 and "uhc_surface_create" in msg and name in msg, (rc, msg)
    assert over.get("out") is False or h.value is None  # no handle is left behind
    L.uhc_surface_free(None)  # freeing nothing is fine


def _metrics(L, **over):
    a = {k: FAKE for k in METRICS_ARGS if k.startswith("d_")}
    a.update(stream=None, surf=FAKE, n_seq=0, row_cap=8, pos_stride=C.c_int64(168), quat_stride=C.c_int64(168), n_rows_total=C.c_int64(16),
             floor_z=C.c_double(0.0), h_bad=None)
    a.update(over)
    rc = L.uhc_surface_metrics(*[a[k] for k in METRICS_ARGS])
    return rc, L.uhc_last_error().decode()


@pytest.mark.parametrize("over,name", [(dict(surf=None), "surf"), (dict(n_seq=-1), "n_seq"), (dict(row_cap=0), "row_cap"), (dict(row_cap=-3), "row_cap"),
                                       (dict(n_rows_total=C.c_int64(-1)), "n_rows_total"), (dict(pos_stride=C.c_int64(2)), "pos_stride"),
                                       (dict(pos_stride=C.c_int64(-168)), "pos_stride"), (dict(quat_stride=C.c_int64(3)), "quat_stride"),
                                       (dict(pos_stride=C.c_int64(2 ** 40)), "pos_stride"), (dict(floor_z=C.c_double(np.nan)), "floor_z"),
                                       (dict(floor_z=C.c_double(np.inf)), "floor_z"), (dict(n_seq=2 ** 31 - 1, row_cap=2 ** 31 - 1), "n_seq")] +
                         [({k: None}, k) for k in METRICS_ARGS if k.startswith("d_") and k != "d_seq_model"])
def test_metrics_refuses_bad_arguments_by_name(L, over, name):
    # (n_seq stays 0 and the handle is a fake: the checks come before the empty return, and nothing reads the handle in front of it.  The two checks
    # that need the handle's n_body -- a stride below a row's width -- are made with a real one: tests/test_gpu_surface_metrics.py)
    rc, msg = _metrics(L, **over)
    assert rc != 0 and "uhc_surface_metrics" in msg and name in msg, (rc, msg)


def test_metrics_of_no_sequence_succeed_without_a_launch(L):
    assert _metrics(L)[0] == 0 and _metrics(L, d_seq_model=None)[0] == 0
    h = C.c_int32(5)
    assert _metrics(L, h_bad=C.byref(h))[0] == 0 and h.value == 0


def _pose(L, **over):
    a = {k: FAKE for k in POSE_ARGS if k.startswith("d_")}
    a.update(stream=None, phase=1, n_env=0, nbody=25, row_cap=8)
    a.update(over)
    rc = L.uhc_eval_record_pose(*[a[k] for k in POSE_ARGS])
    return rc, L.uhc_last_error().decode()


@pytest.mark.parametrize("over,name", [(dict(phase=2), "phase"), (dict(phase=-1), "phase"), (dict(n_env=-1), "n_env"), (dict(nbody=24), "nbody"),
                                       (dict(row_cap=0), "row_cap"), (dict(row_cap=-2), "row_cap")] +
                         [({k: None}, k) for k in POSE_ARGS if k.startswith("d_")])
def test_record_pose_refuses_bad_arguments_by_name(L, over, name):
    rc, msg = _pose(L, **over)
    assert rc != 0 and "uhc_eval_record_pose" in msg and name in msg, (rc, msg)


def test_record_pose_with_no_envs_succeeds_and_takes_no_done_in_phase_0(L):
    assert _pose(L)[0] == 0 and _pose(L, phase=0, d_done=None)[0] == 0 and _pose(L, nbody=27)[0] == 0


def test_header_declares_them_and_the_abi_is_still_11(L):
    from uhc_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uhc_amd.h")).read(), flags=re.S)
    for name in ("uhc_surface_create", "uhc_surface_free", "uhc_surface_metrics", "uhc_eval_record_pose"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert int(re.search(r"#define UHC_ABI_VERSION (\d+)", header).group(1)) == 11
    assert L.uhc_abi_version() == 11
    for name, args in (("uhc_surface_create", CREATE_ARGS), ("uhc_surface_metrics", METRICS_ARGS), ("uhc_eval_record_pose", POSE_ARGS)):
        decl = re.search(r"\b" + name + r"\s*\((.*?)\);", header, flags=re.S).group(1)
        assert [re.search(r"(\w+)\s*$", p).group(1) for p in decl.split(",")] == args
    # the header's export table still equals the library's
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted({l.split()[-1] for l in dyn.splitlines() if " T " in l and l.split()[-1].startswith("uhc_")})
    assert exported == sorted(_lib.SYMBOLS), sorted(set(exported) ^ set(_lib.SYMBOLS))
    declared = sorted(set(re.findall(r"\b(uhc_\w+)\s*\(", header)))
    assert declared == exported, sorted(set(declared) ^ set(exported))


def test_surface_refuses_models_of_different_topology():
    # (refused in Python, before any table travels: no device needed)
    from uhc_amd import eval_ops as EO
    body, zero = np.array([0, 1, 1], dtype=np.int32), np.zeros(3)
    with pytest.raises(ValueError, match="hull vertices"):
        EO.Surface([(np.zeros((3, 3)), body, zero), (np.zeros((4, 3)), np.array([0, 1, 1, 1], dtype=np.int32), np.zeros(4))])
    with pytest.raises(ValueError, match="other bodies"):
        EO.Surface([(np.zeros((3, 3)), body, zero), (np.zeros((3, 3)), np.array([0, 0, 1], dtype=np.int32), zero)])
    with pytest.raises(ValueError, match="no model"):
        EO.Surface([])


def test_config_leaves_the_surface_metrics_off_by_default_and_refuses_what_is_no_bool(tmp_path):
    import yaml
    from uhc_amd.utils.config_utils.copycat_config import Config
    assert Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path)).eval_surface is False
    shipped = yaml.safe_load(open(os.path.join(ROOT, "config", "uhc_amd", "copycat_mi355x.yml")))
    for value in (True, False):
        assert Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path), cfg_dict=dict(shipped, eval_surface=value)).eval_surface is value
    for value in ("device", 1, 0, "true", None):
        with pytest.raises(ValueError, match="eval_surface"):
            Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path), cfg_dict=dict(shipped, eval_surface=value))
