"""CPU: the SMPL body mesh without a GPU.  (1) uhc_amd/csrc/uhc_smpl_mesh_math.h -- the rotation formula, the chain, the feature layout and the tile index
maps uhc_smpl_mesh.hip computes with -- compiled for the host (tests/smpl_mesh_probe.cpp, the matrix product as plain loops over the operands the maps hand
out) against smpl_mesh.lbs_numpy and smpl_eval's compute_* functions; (2) lbs_numpy against the existing pose_body, SMPL_Parser's zero-pose functions against
SMPLBody, the model loader; (3) the C-ABI surface of uhc_smpl_mesh_create / uhc_smpl_mesh: every refusal comes before the first HIP call."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

from tests import probe_build
from tests import smpl_mesh_cases as MC
from uhc_amd.smpllib import smpl_mesh as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)  # a non-null "device pointer": every call here is refused or has nothing to do


def build_probe():
    """tests/smpl_mesh_probe.cpp + the two math headers -> uhc_amd/csrc/build/smpl_mesh_probe.so with the host compiler: no hipcc, no HIP header."""
    return probe_build.build_probe("smpl_mesh_probe.so", ["tests/smpl_mesh_probe.cpp"], ["uhc_amd/csrc/uhc_smpl_mesh_math.h", "uhc_amd/csrc/uhc_surface_math.h"],
                                   probe_build.NO_CONTRACT)


@pytest.fixture(scope="module")
def probe():
    P = C.CDLL(build_probe())
    for f in (P.uhc_smpl_mesh_probe_map, P.uhc_smpl_mesh_probe_b_index, P.uhc_smpl_mesh_probe_pack):
        f.restype = C.c_long
    return P


def _ptr(x):
    return x.ctypes.data_as(C.c_void_p) if x is not None else None


def probe_seq(P, model, beta, pose, trans, floor_z):
    """-> {vertices, joints, row_out, zmin, seq_means} of one sequence, SENTINEL where the probe wrote nothing, and bad"""
    V, T = model["v_template"].shape[0], pose.shape[0]
    tabs = [np.ascontiguousarray(model[k], dtype=np.float64) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")]
    parents = np.ascontiguousarray(model["parents"], dtype=np.int32)
    beta, pose, trans = (np.ascontiguousarray(a, dtype=np.float64) for a in (beta, pose, trans))
    out = dict(vertices=np.full((T, V, 3), MC.SENTINEL), joints=np.full((T, 24, 3), MC.SENTINEL), row_out=np.full((T, 4), MC.SENTINEL), zmin=np.full(T, MC.SENTINEL),
               seq_means=np.full(4, MC.SENTINEL))
    bad = P.uhc_smpl_mesh_probe_seq(C.c_int(V), *[_ptr(t) for t in tabs], _ptr(parents), _ptr(beta), _ptr(pose), _ptr(trans), C.c_int(T), C.c_double(floor_z),
                                    _ptr(out["vertices"]), _ptr(out["joints"]), _ptr(out["row_out"]), _ptr(out["zmin"]), _ptr(out["seq_means"]))
    return out, bad


def probe_case(P, c):
    """the probe over every sequence of a case, laid out over the global rows like the case's expectation"""
    e = c["expected"]
    got = {k: np.full_like(v, MC.SENTINEL) for k, v in e.items()}
    bad = 0
    for s, T in enumerate(c["rows"]):
        g = slice(int(c["start"][s]), int(c["start"][s]) + T)
        out, b = probe_seq(P, c["models"][c["seq_model"][s]], c["betas"][s], c["pose"][g], c["trans"][g], c["floor_z"])
        for k in ("vertices", "joints", "row_out", "zmin"):
            got[k][g] = out[k]
        got["seq_means"][s] = out["seq_means"]
        bad += b
    return got, bad


ALL = ("vertices", "joints", "row_out", "zmin", "seq_means")


# ---------------------------------------------------------------- 1. the arithmetic and the maps
@pytest.mark.parametrize("V", MC.VERTS)
def test_probe_matches_lbs_numpy(probe, V):
    for dense in (False, True):
        c = MC.make_case(V, (MC.TILE_ROWS + 2, 1, 3), seed=int(dense), dense_weights=dense, floor_z=0.25 if dense else 0.0)
        got, bad = probe_case(probe, c)
        assert bad == 0
        MC.assert_matches(got, c["expected"], ALL, where=f"V={V} dense={dense}")
        assert np.isnan(got["seq_means"][1, 1]) and got["row_out"][int(c["start"][1]), 1] == MC.SENTINEL  # one row: no pair, the mean over nothing


def test_probe_gives_a_bad_row_nan_and_leaves_the_others_alone(probe):
    c = MC.make_case(17, (5,))
    g0 = int(c["start"][0])
    pose, trans = c["pose"][g0:g0 + 5].copy(), c["trans"][g0:g0 + 5].copy()
    ref, _ = probe_seq(probe, c["models"][0], c["betas"][0], pose, trans, 0.0)
    pose[2, 40] = np.nan
    out, bad = probe_seq(probe, c["models"][0], c["betas"][0], pose, trans, 0.0)
    assert bad == 1 and np.isnan(out["row_out"][2]).all() and np.isnan(out["row_out"][1, 1]) and np.isnan(out["vertices"][2]).all() and np.isnan(out["zmin"][2])
    keep = np.ones((5, 4), dtype=bool)
    keep[2], keep[1, 1] = False, False
    assert np.array_equal(out["row_out"][keep], ref["row_out"][keep])
    for k in ("vertices", "joints", "zmin"):
        assert np.array_equal(np.delete(out[k], 2, axis=0), np.delete(ref[k], 2, axis=0))


def test_rotation_is_the_identity_at_zero_and_smplx_formula_elsewhere(probe):
    R = np.zeros(9)
    probe.uhc_smpl_mesh_probe_rodrigues(_ptr(np.zeros(3)), _ptr(R))
    assert np.array_equal(R, np.eye(3).ravel())  # exactly: the direction is 0
    assert np.array_equal(SM.rodrigues(np.zeros(3)), np.eye(3))
    from scipy.spatial.transform import Rotation as sRot
    rng = np.random.default_rng(5)
    for r in rng.normal(size=(20, 3)):
        probe.uhc_smpl_mesh_probe_rodrigues(_ptr(np.ascontiguousarray(r)), _ptr(R))
        np.testing.assert_allclose(R.reshape(3, 3), SM.rodrigues(r), atol=1e-15, rtol=0)
        np.testing.assert_allclose(R.reshape(3, 3), sRot.from_rotvec(r).as_matrix(), atol=1e-7, rtol=0)  # (smplx's 1e-8 in the angle)


def test_index_maps_cover_every_operand_and_result_exactly_once(probe):
    m = lambda which, x=0, y=0: int(probe.uhc_smpl_mesh_probe_map(which, x, y))
    for p in (0, 1, 51):
        assert sorted((m(0, 0, l), m(1, p, l)) for l in range(64)) == [(r, 4 * p + k) for r in range(16) for k in range(4)]  # A: (row, k)
        assert sorted((m(2, p, l), m(3, 0, l)) for l in range(64)) == [(4 * p + k, v) for k in range(4) for v in range(16)]  # B: (k, vertex)
    assert sorted((m(4, l, i), m(5, l)) for l in range(64) for i in range(4)) == [(r, v) for r in range(16) for v in range(16)]  # C / D: (row, vertex)
    assert sorted(4 * p + k for p in range(52) for k in range(4)) == list(range(208))
    for l in range(64):  # the next row of (lane, register) is the same vertex, one row on -- or beyond the tile, from row 15
        for i in range(4):
            nl, nr = m(6, l), m(7, l, i)
            assert m(5, nl) == m(5, l)
            assert (nr == 4 and m(4, l, i) == 15) or m(4, nl, nr) == m(4, l, i) + 1
    # the feature: k <-> (joint 1 .. 23, element), 207 of them
    ks = [m(8, j, e) for j in range(1, 24) for e in range(9)]
    assert ks == list(range(207)) and all((m(9, k), m(10, k)) == (1 + k // 9, k % 9) for k in ks)
    # row tiles own 15 rows and overlap by one; the cases' row counts sit on THAT edge (their TILE_ROWS is the header's UHC_SM_OWNED, read through the probe)
    assert MC.TILE_ROWS == m(12, 1) - m(12, 0) and len({m(0, 0, l) for l in range(64)}) == MC.TILE_ROWS + 1
    assert m(11, MC.TILE_ROWS) == 1 and m(11, MC.TILE_ROWS + 1) == 2 and set(MC.ROWS) >= {1, 2, MC.TILE_ROWS - 1, MC.TILE_ROWS, MC.TILE_ROWS + 1, 2 * MC.TILE_ROWS + 1}
    assert [m(11, T) for T in (0, 1, 15, 16, 30, 31)] == [0, 1, 1, 2, 2, 3] and [m(12, t) for t in range(3)] == [0, 15, 30]
    assert [m(13, V) for V in (1, 16, 17, 6890)] == [1, 1, 2, 431]
    # a wave's transforms in LDS: 24 x 12 x 16 slots, none shared
    slots = {m(14, j, c) + row for j in range(24) for c in range(12) for row in range(16)}
    assert len(slots) == 24 * 12 * 16 and max(slots) < 24 * 193


def test_packed_posedirs_hold_every_entry_once_and_zeros_elsewhere(probe):
    V = 17
    pd = np.arange(1, V * 3 * 207 + 1, dtype=np.float64).reshape(V, 3, 207)
    n = int(probe.uhc_smpl_mesh_probe_pack(V, None, None))
    assert n == 2 * 3 * 208 * 16
    out = np.full(n, -1.0)
    probe.uhc_smpl_mesh_probe_pack(V, _ptr(pd), _ptr(out))
    assert sorted(out[out != 0]) == sorted(pd.ravel()) and (out != 0).sum() == pd.size
    for v, c, k in ((0, 0, 0), (16, 2, 206), (5, 1, 100)):
        assert out[int(probe.uhc_smpl_mesh_probe_b_index(v // 16, c, k, v % 16))] == pd[v, c, k]
    # one K-step of one tile and coordinate: 64 neighbouring doubles, in lane order
    base = int(probe.uhc_smpl_mesh_probe_b_index(1, 2, 8, 0))
    assert [int(probe.uhc_smpl_mesh_probe_b_index(1, 2, 8 + (l >> 4), l & 15)) for l in range(64)] == list(range(base, base + 64))


# ---------------------------------------------------------------- 2. the host functions
def test_lbs_numpy_without_pose_blend_shapes_is_pose_body():
    from uhc_amd.smpllib.smpl_robot import pose_body
    m = dict(MC.synthetic_model(50, 3))
    m["posedirs"] = np.zeros_like(m["posedirs"])
    rng = np.random.default_rng(2)
    beta = rng.normal(size=10)
    rest, joints = SM.lbs_numpy(m, np.zeros((1, 72)), beta)
    for pose in MC.random_poses(rng, 4):
        vert, _ = SM.lbs_numpy(m, pose[None], beta)
        np.testing.assert_allclose(vert[0], pose_body(rest[0], joints[0], m["weights"], pose), atol=1e-6, rtol=0)  # (they differ by smplx's 1e-8 in the angle)


def _write_model(path, tabs):
    if str(path).endswith(".npz"):
        np.savez(path, **tabs)
    else:
        with open(path, "wb") as f:
            pickle.dump(tabs, f)


def test_load_smpl_model_reads_both_formats_both_layouts_and_sparse_regressors(tmp_path):
    import scipy.sparse as sp
    tabs = MC.synthetic_tables(17, 1)
    want = SM.model_from_tables(tabs)
    variants = {"a.npz": tabs, "b.pkl": tabs, "c.pkl": dict(tabs, J_regressor=sp.csc_matrix(tabs["J_regressor"])),
                "d.npz": dict(tabs, posedirs=tabs["posedirs"].reshape(17 * 3, 207).T.copy()),
                "e.pkl": dict(tabs, shapedirs=np.concatenate([tabs["shapedirs"], np.ones((17, 3, 290))], axis=2))}
    for name, t in variants.items():
        _write_model(tmp_path / name, t)
        got = SM.load_smpl_model(tmp_path / name)
        for k, v in want.items():
            assert np.array_equal(got[k], v) and got[k].dtype == v.dtype, (name, k)
    assert want["parents"][0] == -1 and want["parents"].dtype == np.int32 and want["shapedirs"].shape == (17, 3, 10)
    # a directory: the gender chooses the file
    d = tmp_path / "smpl"
    d.mkdir()
    _write_model(d / "SMPL_MALE.pkl", MC.synthetic_tables(17, 2))
    assert np.array_equal(SM.load_smpl_model(d, "male")["v_template"], MC.synthetic_model(17, 2)["v_template"])
    assert np.array_equal(SM.load_smpl_model(d, 1)["v_template"], MC.synthetic_model(17, 2)["v_template"])
    with pytest.raises(FileNotFoundError, match="SMPL_NEUTRAL"):
        SM.load_smpl_model(d, "neutral")


def test_load_smpl_model_refuses_a_file_without_posedirs_and_other_bodies(tmp_path):
    tabs = MC.synthetic_tables(17, 1)
    _write_model(tmp_path / "zero_pose_only.npz", {k: v for k, v in tabs.items() if k != "posedirs"})
    with pytest.raises(ValueError, match="posedirs"):
        SM.load_smpl_model(tmp_path / "zero_pose_only.npz")
    _write_model(tmp_path / "smplh.pkl", dict(tabs, posedirs=np.zeros((17, 3, 459))))
    with pytest.raises(ValueError, match="SMPL-H"):
        SM.load_smpl_model(tmp_path / "smplh.pkl")
    bad_tree = tabs["kintree_table"].copy()
    bad_tree[0, 3] = 7
    _write_model(tmp_path / "tree.pkl", dict(tabs, kintree_table=bad_tree))
    with pytest.raises(ValueError, match="kintree_table"):
        SM.load_smpl_model(tmp_path / "tree.pkl")


def test_parser_zero_pose_functions_agree_with_smplbody_on_the_same_file(tmp_path):
    from uhc_amd.smpllib.smpl_robot import SMPL_PARENTS, SMPLBody
    from uhc_amd.smpllib.smpl_mujoco import SMPL_BONE_ORDER_NAMES
    _write_model(tmp_path / "SMPL_NEUTRAL.pkl", MC.synthetic_tables(50, 4))
    beta = np.random.default_rng(0).normal(size=16)
    verts, joints, W = SMPLBody(str(tmp_path))(beta[:10], 0)
    from uhc.smpllib.smpl_parser import SMPL_Parser  # (the reference's import line, through the alias)
    assert SMPL_Parser is SM.SMPL_Parser
    P = SMPL_Parser(str(tmp_path), gender="neutral")
    out = P.get_mesh_offsets(beta)
    assert len(out) == 11
    np.testing.assert_allclose(out[0], verts, atol=1e-14, rtol=0)
    np.testing.assert_allclose(out[1], joints, atol=1e-14, rtol=0)
    assert np.array_equal(out[2], W) and out[3] == list(SMPL_BONE_ORDER_NAMES)
    names = out[3]
    for c, p in enumerate(SMPL_PARENTS):
        np.testing.assert_allclose(out[4][names[c]], joints[c] - joints[p] if c > 0 else joints[c], atol=1e-14, rtol=0)
        assert out[5][names[c]] == (names[p] if p >= 0 else None)
    offsets, parents, channels, ranges = P.get_offsets(beta)
    assert channels == ["z", "y", "x"] and np.array_equal(offsets[names[0]], np.zeros(3)) and parents[names[4]] == names[1]
    np.testing.assert_allclose(offsets[names[7]], joints[7] - joints[4], atol=1e-14, rtol=0)
    assert np.array_equal(ranges["L_Elbow"], np.tile([-4 * np.pi, 4 * np.pi], (3, 1))) and np.array_equal(ranges["L_Knee"], np.tile([-np.pi, np.pi], (3, 1)))
    flat = P.get_mesh_offsets(beta, flatfoot=True)[0]
    feet = verts[:, 1] < verts[:, 1].min() + 0.01
    assert np.allclose(flat[feet, 1], verts[feet, 1].mean()) and np.array_equal(flat[~feet], out[0][~feet])
    with pytest.raises(ValueError, match="device tensors"):
        P.get_joints_verts(np.zeros((1, 72)))


# ---------------------------------------------------------------- 3. the C-ABI surface
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from uhc_amd import _lib
    return _lib.lib()


CREATE_ARGS = ["n_vert", "n_models", "h_v_template", "h_shapedirs", "h_posedirs", "h_J_regressor", "h_weights", "h_parents", "out"]
MESH_ARGS = ["stream", "mesh", "n_seq", "d_seq_start", "d_seq_rows", "row_cap", "d_seq_model", "d_betas", "d_pose_aa", "pose_stride", "d_trans", "trans_stride",
             "n_rows_total", "floor_z", "d_vert", "d_joints", "d_row_out", "d_seq_means", "d_row_zmin", "d_bad", "h_bad"]
TABLES = {"h_v_template": "v_template", "h_shapedirs": "shapedirs", "h_posedirs": "posedirs", "h_J_regressor": "J_regressor", "h_weights": "weights"}


def _create(L, n_vert=3, n_models=1, parents=None, poison=None, null=(), out=True):
    m = MC.synthetic_model(3, 0)
    tabs = {h: np.ascontiguousarray(m[k], dtype=np.float64).copy() for h, k in TABLES.items()}
    if poison:
        tabs[poison[0]].reshape(-1)[-1] = poison[1]
    par = np.array(m["parents"] if parents is None else parents, dtype=np.int32)
    h = C.c_void_p(0x1234)
    a = dict(n_vert=n_vert, n_models=n_models, h_parents=_ptr(par), out=C.byref(h) if out else None, **{k: _ptr(v) for k, v in tabs.items()})
    for k in null:
        a[k] = None
    rc = L.uhc_smpl_mesh_create(*[a[k] for k in CREATE_ARGS])
    return rc, L.uhc_last_error().decode(), h


def _tree(j, p):
    from uhc_amd.smpllib.smpl_robot import SMPL_PARENTS
    t = list(SMPL_PARENTS)
    t[j] = p
    return t


@pytest.mark.parametrize("over,name", [(dict(n_vert=0), "n_vert"), (dict(n_vert=65536), "n_vert"), (dict(n_models=0), "n_models"), (dict(n_models=-2), "n_models"),
                                       (dict(parents=_tree(0, 0)), "h_parents"), (dict(parents=_tree(5, 5)), "h_parents"), (dict(parents=_tree(5, 9)), "h_parents"),
                                       (dict(parents=_tree(5, -1)), "h_parents"), (dict(parents=_tree(23, 24)), "h_parents"), (dict(out=False), "out")] +
                         [(dict(poison=(k, bad)), k) for k in TABLES for bad in (np.nan, np.inf)] + [(dict(null=(k,)), k) for k in list(TABLES) + ["h_parents"]])
def test_create_refuses_bad_tables_by_name(L, over, name):
    # (every refusal comes before the first HIP call: this runs on a machine without a GPU)
    rc, msg, h = _create(L, **over)
    assert rc != 0 and "uhc_smpl_mesh_create" in msg and name in msg, (rc, msg)
    assert over.get("out") is False or h.value is None  # no handle is left behind
    L.uhc_smpl_mesh_free(None)  # freeing nothing is fine


def _mesh(L, **over):
    a = {k: FAKE for k in MESH_ARGS if k.startswith("d_")}
    a.update(stream=None, mesh=FAKE, n_seq=0, row_cap=8, pose_stride=C.c_int64(72), trans_stride=C.c_int64(3), n_rows_total=C.c_int64(16), floor_z=C.c_double(0.0),
             h_bad=None)
    a.update(over)
    rc = L.uhc_smpl_mesh(*[a[k] for k in MESH_ARGS])
    return rc, L.uhc_last_error().decode()


OUTPUTS = ("d_vert", "d_joints", "d_row_out", "d_seq_means", "d_row_zmin")


@pytest.mark.parametrize("over,name", [(dict(mesh=None), "mesh"), (dict(n_seq=-1), "n_seq"), (dict(n_seq=2 ** 31 - 1, row_cap=2 ** 31 - 1), "n_seq"), (dict(row_cap=0), "row_cap"),
                                       (dict(n_rows_total=C.c_int64(-1)), "n_rows_total"), (dict(pose_stride=C.c_int64(71)), "pose_stride"),
                                       (dict(trans_stride=C.c_int64(2)), "trans_stride"), (dict(pose_stride=C.c_int64(2 ** 40)), "pose_stride"),
                                       (dict(floor_z=C.c_double(np.nan)), "floor_z"), (dict(floor_z=C.c_double(-np.inf)), "floor_z"),
                                       ({k: None for k in OUTPUTS}, "every output")] +
                         [({k: None}, k) for k in ("d_seq_start", "d_seq_rows", "d_betas", "d_pose_aa", "d_trans", "d_bad")])
def test_mesh_refuses_bad_arguments_by_name(L, over, name):
    rc, msg = _mesh(L, **over)
    assert rc != 0 and "uhc_smpl_mesh" in msg and name in msg, (rc, msg)


def test_mesh_of_no_sequence_succeeds_without_a_launch_and_every_output_is_optional(L):
    assert _mesh(L)[0] == 0 and _mesh(L, d_seq_model=None)[0] == 0
    for keep in OUTPUTS:
        assert _mesh(L, **{k: None for k in OUTPUTS if k != keep})[0] == 0
    h = C.c_int32(5)
    assert _mesh(L, h_bad=C.byref(h))[0] == 0 and h.value == 0


def test_header_declares_them_and_the_abi_is_still_11(L):
    from uhc_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uhc_amd.h")).read(), flags=re.S)
    assert int(re.search(r"#define UHC_ABI_VERSION (\d+)", header).group(1)) == 11 and L.uhc_abi_version() == 11
    for name, args in (("uhc_smpl_mesh_create", CREATE_ARGS), ("uhc_smpl_mesh_free", ["mesh"]), ("uhc_smpl_mesh", MESH_ARGS)):
        assert name in _lib.SYMBOLS and hasattr(L, name)
        decl = re.search(r"\b" + name + r"\s*\((.*?)\);", header, flags=re.S).group(1)
        assert [re.search(r"(\w+)\s*$", p).group(1) for p in decl.split(",")] == args
    import __graft_entry__ as g
    assert "uhc_smpl_mesh.hip" in g.HIP_SOURCES and "uhc_smpl_mesh.hip" not in g.STEP_KERNEL_UNITS


def test_smplmesh_refuses_models_of_different_topology():
    from uhc_amd import eval_ops as EO
    with pytest.raises(ValueError, match="vertices"):
        EO.SmplMesh([MC.synthetic_model(15, 0), MC.synthetic_model(16, 0)])
    with pytest.raises(ValueError, match="no model"):
        EO.SmplMesh([])


def test_config_leaves_the_mesh_metrics_off_by_default_and_takes_a_directory_only(tmp_path):
    import yaml
    from uhc_amd.utils.config_utils.copycat_config import Config
    assert Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path)).eval_mesh is False
    shipped = yaml.safe_load(open(os.path.join(ROOT, "config", "uhc_amd", "copycat_mi355x.yml")))
    for value in (False, "data/smpl"):
        assert Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path), cfg_dict=dict(shipped, eval_mesh=value)).eval_mesh == value
    for value in (True, 1, 0, "", None):
        with pytest.raises(ValueError, match="eval_mesh"):
            Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path), cfg_dict=dict(shipped, eval_mesh=value))
    with pytest.raises(ValueError, match="eval_surface"):  # the two write the same result keys
        Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path), cfg_dict=dict(shipped, eval_mesh="data/smpl", eval_surface=True))
    assert Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path), cfg_dict=dict(shipped, eval_surface=True)).eval_mesh is False


def test_host_fix_height_is_unchanged_and_the_device_variant_wants_the_full_files(tmp_path):
    from uhc_amd.smpllib.smpl_robot import make_fix_height, pose_body
    m = MC.synthetic_model(50, 4)
    prov = lambda betas, gender: (SM.lbs_numpy(m, np.zeros((1, 72)), betas)[0][0], SM.lbs_numpy(m, np.zeros((1, 72)), betas)[1][0], m["weights"])
    rng = np.random.default_rng(1)
    pose, betas, trans = MC.random_poses(rng, 3), rng.normal(size=10), rng.normal(size=(3, 3))
    out = make_fix_height(prov)(pose, betas, trans, "neutral")
    v, j, w = prov(betas, 0)
    assert np.array_equal(out[:, 2], trans[:, 2] - (pose_body(v, j, w, pose[0]) + trans[0])[:, 2].min())
    with pytest.raises(ValueError, match="MeshBodyProvider"):
        make_fix_height(prov, device=True)
