"""GPU: uhc_smpl_mesh (uhc_amd/csrc/uhc_smpl_mesh.hip) against smpl_mesh.lbs_numpy + smpl_eval's compute_* and against the host probe
(tests/smpl_mesh_probe.cpp), at the tolerances of tests/smpl_mesh_cases.py: vertices and joints 1e-10 m (the forward-error bound of the ~250-term float64
sums at these magnitudes is ~1e-12 m), metrics 1e-6 mm.  Shapes are the smallest at which the kernel can go wrong: a row tile owns 15 rows and holds 16, a
vertex tile 16 vertices, a workgroup four row tiles."""
import numpy as np
import pytest
import torch

from tests import smpl_mesh_cases as MC
from tests.test_smpl_mesh_cpu import ALL, probe_case
from tests.test_smpl_mesh_cpu import probe  # noqa: F401  (the fixture)
from uhc_amd.smpllib import smpl_mesh as SM

pytestmark = pytest.mark.gpu
R = MC.TILE_ROWS
_MESHES = {}


def mesh_of(c):
    """one device handle per set of models (the cases are cached, so their model lists are the same objects)"""
    from uhc_amd import eval_ops as EO
    key = id(c["models"])
    if key not in _MESHES:
        _MESHES[key] = (EO.SmplMesh(c["models"]), c["models"])
    return _MESHES[key][0]


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def run(c, want=("vertices", "joints", "metrics", "zmin"), pose=None, trans=None, rows=None, start=None, seq_model=None, sentinel=True, **kw):
    """uhc_smpl_mesh on a case -> {name: numpy array}; the outputs are handed in filled with SENTINEL"""
    from uhc_amd import eval_ops as EO
    mesh = mesh_of(c)
    pose = dev(c["pose"]) if pose is None else pose
    trans = dev(c["trans"]) if trans is None else trans
    rows = dev(np.array(c["rows"] if rows is None else rows, dtype=np.int32))
    start = dev(np.array(c["start"] if start is None else start, dtype=np.int64))
    seq_model = dev(np.array(c["seq_model"] if seq_model is None else seq_model, dtype=np.int32))
    n, S, V = pose.shape[0], rows.numel(), c["V"]
    shapes = {"vertices": (n, V, 3), "joints": (n, 24, 3), "row_out": (n, 4), "seq_means": (S, 4), "zmin": (n,)}
    out = {k: torch.full(s, MC.SENTINEL, dtype=torch.float64, device="cuda") for k, s in shapes.items()} if sentinel else None
    kw.setdefault("row_cap", max(max(c["rows"]), 1))
    kw.setdefault("floor_z", c["floor_z"])
    res = EO.smpl_mesh(mesh, pose, trans, start, rows, dev(c["betas"])[:S].contiguous(), seq_model=seq_model, want=want, out=out, wait=True, **kw)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}


@pytest.mark.parametrize("V", MC.VERTS)
def test_device_matches_lbs_numpy_and_the_probe_on_every_vertex_count(probe, V):  # noqa: F811
    # sequences of different lengths in one call: tiles straddle sequence ends, neighbours in a workgroup have other betas and another model
    for dense in (False, True):
        c = MC.make_case(V, (R + 2, 1, 3), seed=int(dense), dense_weights=dense, floor_z=0.25 if dense else 0.0)
        got = run(c)
        assert got["bad"] == 0
        MC.assert_matches(got, c["expected"], ALL, where=f"V={V} dense={dense} vs lbs_numpy")
        MC.assert_matches(got, probe_case(probe, c)[0], ALL, where=f"V={V} dense={dense} vs probe")


def test_every_row_count_around_the_tile(probe):  # noqa: F811
    c = MC.make_case(17, MC.ROWS)  # 1, 2, R - 1, R, R + 1, R + 2 (= 16 + 1), 2 R + 1, 2 R + 3 (= 2 x 16 + 1): eight sequences, two workgroups and more
    got = run(c)
    assert got["bad"] == 0
    MC.assert_matches(got, c["expected"], ALL, where="rows")
    MC.assert_matches(got, probe_case(probe, c)[0], ALL, where="rows vs probe")
    # the row counts are clamped to row_cap: with a cap of 4 every longer sequence is its first four rows
    cap = run(c, row_cap=4)
    for s, T in enumerate(c["rows"]):
        g0, n = int(c["start"][s]), min(T, 4)
        np.testing.assert_allclose(cap["vertices"][g0:g0 + n], c["expected"]["vertices"][g0:g0 + n], rtol=0, atol=MC.VERT_ATOL)
        assert (cap["vertices"][g0 + n:g0 + T] == MC.SENTINEL).all() and (cap["row_out"][g0 + n:g0 + T] == MC.SENTINEL).all()
        np.testing.assert_allclose(cap["row_out"][g0:g0 + n, [0, 2, 3]], c["expected"]["row_out"][g0:g0 + n, [0, 2, 3]], rtol=0, atol=MC.METRIC_ATOL)
        assert cap["row_out"][g0 + n - 1, 1] == MC.SENTINEL  # the last row of the clamped sequence has no skate


def test_the_real_vertex_count_once():
    c = MC.make_case(6890, (17,), n_models=1)  # 431 vertex tiles, the last with 10 vertices; two row tiles
    got = run(c)
    assert got["bad"] == 0
    MC.assert_matches(got, c["expected"], ALL, where="V=6890")


def test_strides_of_the_pose_converter_and_an_odd_alignment():
    c = MC.make_case(17, (R + 1, 3))
    n = c["n_total"]
    want = run(c)
    # rows 147 + 72 wide (a full_6d block beside the poses), translations in the first columns of a frame-wide row; and both 8 bytes behind a 16-byte boundary
    wide = torch.full((n, 147 + 72), 7.0, dtype=torch.float64, device="cuda")
    wide[:, 147:] = dev(c["pose"])
    frame = torch.full((n, 584), 7.0, dtype=torch.float64, device="cuda")
    frame[:, 5:8] = dev(c["trans"])
    got = run(c, pose=wide[:, 147:], trans=frame[:, 5:8])
    flat = torch.zeros(n * 72 + 1, dtype=torch.float64, device="cuda")
    odd = flat[1:].view(n, 72)
    odd.copy_(dev(c["pose"]))
    tflat = torch.zeros(n * 3 + 1, dtype=torch.float64, device="cuda")
    todd = tflat[1:].view(n, 3)
    todd.copy_(dev(c["trans"]))
    assert odd.data_ptr() % 16 == 8 and todd.data_ptr() % 16 == 8
    got2 = run(c, pose=odd, trans=todd)
    for k in ALL:
        assert np.array_equal(got[k], want[k]) and np.array_equal(got2[k], want[k]), k
    # ... and the converter's own outputs, read where it left them (3-D tensors flattened over sequence and row)
    from uhc_amd.eval_ops import smpl_mesh
    pa, tr = dev(c["pose"]).view(1, n, 72), dev(c["trans"]).view(1, n, 3)
    res = smpl_mesh(mesh_of(c), pa.view(n, 72), tr.view(n, 3), dev(c["start"]), dev(np.array(c["rows"], dtype=np.int32)), dev(c["betas"]),
                    seq_model=dev(c["seq_model"]), want=("rows",), wait=True)
    keep = want["row_out"] != MC.SENTINEL
    assert np.array_equal(res["row_out"].cpu().numpy()[keep], want["row_out"][keep]) and torch.isnan(res["row_out"][~torch.as_tensor(keep).cuda()]).all()


def test_every_output_alone_equals_all_together():
    c = MC.make_case(17, (R + 1, 3))
    full = run(c)
    for want, keys in ((("vertices",), ["vertices"]), (("joints",), ["joints"]), (("rows",), ["row_out"]), (("means",), ["seq_means"]), (("zmin",), ["zmin"]),
                       (("joints", "means"), ["joints", "seq_means"])):
        got = run(c, want=want)
        assert sorted(k for k in got if k != "bad") == sorted(keys)
        for k in keys:
            assert np.array_equal(got[k], full[k]), (want, k)


def test_zero_pose_zero_betas_zero_translation_give_the_template():
    c = MC.make_case(50, (3,), n_models=1)
    n = c["n_total"]
    m = c["models"][0]
    zero = dict(c, betas=np.zeros_like(c["betas"]))
    got = run(zero, want=("vertices", "joints"), pose=torch.zeros(n, 72, dtype=torch.float64, device="cuda"),
              trans=torch.zeros(n, 3, dtype=torch.float64, device="cuda"), rows=[3], start=[0], seq_model=[0])
    for r in range(3):
        np.testing.assert_allclose(got["vertices"][r], m["v_template"], rtol=0, atol=1e-15)  # the feature is exactly 0: no posedirs entry reaches a vertex
        # (joints: a chain of up to nine additions of numbers below 2, each rounded to half an ulp of 2.2e-16, and the eight-term sums of the regressor)
        np.testing.assert_allclose(got["joints"][r], m["J_regressor"] @ m["v_template"], rtol=0, atol=4e-15)


def test_a_nan_row_is_nan_counts_once_and_leaves_the_others_bit_identical():
    c = MC.make_case(17, (R + 2, 3))
    ref = run(c)
    for r_bad in (4, R - 1, R):  # inside a tile, its last own row, the first row of the next tile (the row both tiles hold)
        pose = dev(c["pose"])
        g = int(c["start"][0]) + r_bad
        pose[g, 40] = float("nan")
        got = run(c, pose=pose)
        assert got["bad"] == 1
        assert np.isnan(got["row_out"][g]).all() and np.isnan(got["row_out"][g - 1, 1]) and np.isnan(got["vertices"][g]).all() and np.isnan(got["joints"][g]).all()
        assert np.isnan(got["zmin"][g]) and np.isnan(got["seq_means"][0]).all()
        keep = np.ones_like(ref["row_out"], dtype=bool)
        keep[g], keep[g - 1, 1] = False, False
        assert np.array_equal(got["row_out"][keep], ref["row_out"][keep])
        for k in ("vertices", "joints", "zmin"):
            assert np.array_equal(np.delete(got[k], g, axis=0), np.delete(ref[k], g, axis=0)), k
        assert np.array_equal(got["seq_means"][1], ref["seq_means"][1])
    trans = dev(c["trans"])
    trans[int(c["start"][1]), 2] = float("inf")
    got = run(c, trans=trans)
    assert got["bad"] == 1 and np.isnan(got["row_out"][int(c["start"][1])]).all() and np.array_equal(got["seq_means"][0], ref["seq_means"][0])


def test_sequences_outside_the_rows_are_skipped_and_counted_and_a_bad_model_index_reads_as_model_0():
    c = MC.make_case(17, (R + 2, 3))
    ref = run(c)
    n = c["n_total"]
    for start1 in (n - 2, -1, 2 ** 40):  # three rows from n - 2 would leave the arrays
        got = run(c, start=[int(c["start"][0]), start1])
        assert got["bad"] == 1
        g1 = int(c["start"][1])
        keep = np.ones(n, dtype=bool)
        keep[g1:g1 + 3] = False
        for k in ("vertices", "joints", "row_out", "zmin"):
            assert np.array_equal(got[k][keep], ref[k][keep]) and (got[k][~keep] == MC.SENTINEL).all(), k
        assert (got["seq_means"][1] == MC.SENTINEL).all() and np.array_equal(got["seq_means"][0], ref["seq_means"][0])
    # negative and huge row counts: 0 rows and row_cap rows
    got = run(c, rows=[-5, 3])
    assert got["bad"] == 0 and (got["vertices"][int(c["start"][0])] == MC.SENTINEL).all() and np.isnan(got["seq_means"][0]).all()
    # sequence 1 is model 1 in the case: out of range it is model 0, which is what the case with [0, 0] gives
    as0 = run(c, seq_model=[0, 0])
    assert not np.array_equal(as0["vertices"], ref["vertices"])
    for bad_model in (2, -1, 2 ** 31 - 1):
        got = run(c, seq_model=[0, bad_model])
        for k in ALL:
            assert np.array_equal(got[k], as0[k]), (bad_model, k)


def test_no_sequence_launches_nothing_and_two_calls_are_bit_identical():
    from uhc_amd import eval_ops as EO
    c = MC.make_case(17, MC.ROWS)
    e = lambda dt: torch.zeros(0, dtype=dt, device="cuda")
    res = EO.smpl_mesh(mesh_of(c), dev(c["pose"]), dev(c["trans"]), e(torch.int64), e(torch.int32), torch.zeros(0, 10, dtype=torch.float64, device="cuda"), wait=True)
    assert res["bad"] == 0 and torch.isnan(res["row_out"]).all() and res["seq_means"].shape == (0, 4)
    a, b = run(c), run(c)
    for k in ALL:
        assert a[k].tobytes() == b[k].tobytes(), k  # (bit for bit, the NaN of a one-row sequence's mean skate included)


def test_more_one_row_sequences_than_a_grid_dimension_holds():
    from uhc_amd import eval_ops as EO
    c = MC.make_case(1, (3,), n_models=1)
    n = 65540  # beyond 65 535: the sequence index rides in blockIdx.x of every kernel
    rng = np.random.default_rng(7)
    pose, betas, trans = MC.random_poses(rng, n), rng.normal(size=(n, 10)), rng.normal(size=(n, 3))
    res = EO.smpl_mesh(mesh_of(c), dev(pose), dev(trans), torch.arange(n, dtype=torch.int64, device="cuda"), torch.ones(n, dtype=torch.int32, device="cuda"),
                       dev(betas), want=("vertices", "joints", "means"), row_cap=1, wait=True)
    ev, ej = SM.lbs_numpy(c["models"][0], pose, betas, trans)
    assert res["bad"] == 0
    np.testing.assert_allclose(res["vertices"].cpu().numpy(), ev, rtol=0, atol=MC.VERT_ATOL)
    np.testing.assert_allclose(res["joints"].cpu().numpy(), ej, rtol=0, atol=MC.VERT_ATOL)
    contact = (ev[:, :, 2] <= 0).sum(axis=1).astype(np.float64)
    assert np.array_equal(res["seq_means"][:, 3].cpu().numpy(), contact) and torch.isnan(res["seq_means"][:, 1]).all()


# ---------------------------------------------------------------- through the layers
def test_parser_get_joints_verts_on_device_tensors(tmp_path):
    import pickle
    with open(tmp_path / "SMPL_FEMALE.pkl", "wb") as f:
        pickle.dump(MC.synthetic_tables(50, 6), f)
    from uhc.smpllib.smpl_parser import SMPL_Parser
    P = SMPL_Parser(str(tmp_path), gender="female")
    rng = np.random.default_rng(1)
    pose, betas16, trans = MC.random_poses(rng, 5), rng.normal(size=(1, 16)), rng.normal(size=(5, 3))
    v, j = P.get_joints_verts(dev(pose).view(5, 24, 3), th_betas=dev(betas16), th_trans=dev(trans))  # (reshaped to (-1, 72); 16 betas cut to 10)
    ev, ej = SM.lbs_numpy(P.model, pose, betas16[0, :10], trans)
    assert v.is_cuda and v.shape == (5, 50, 3) and j.shape == (5, 24, 3)
    np.testing.assert_allclose(v.cpu().numpy(), ev, rtol=0, atol=MC.VERT_ATOL)
    np.testing.assert_allclose(j.cpu().numpy(), ej, rtol=0, atol=MC.VERT_ATOL)
    # a body per pose, no translation, no betas
    b5 = rng.normal(size=(5, 10))
    v, j = P.get_joints_verts(dev(pose), th_betas=dev(b5))
    ev, ej = SM.lbs_numpy(P.model, pose, b5)
    np.testing.assert_allclose(v.cpu().numpy(), ev, rtol=0, atol=MC.VERT_ATOL)
    v, _ = P.get_joints_verts(dev(pose))
    np.testing.assert_allclose(v.cpu().numpy(), SM.lbs_numpy(P.model, pose)[0], rtol=0, atol=MC.VERT_ATOL)


def test_mesh_metrics_of_record_on_a_hand_made_record():
    from uhc_amd import eval_ops as EO
    from uhc_amd.sim import load_asset_model
    model = load_asset_model()
    rng = np.random.default_rng(4)
    n_env, cap = 3, R + 3
    rec = EO.Record(n_env, cap, 76, "cuda")
    q = np.zeros((n_env, cap, 76))
    q[:, :, :2] = rng.normal(scale=0.3, size=(n_env, cap, 2))
    q[:, :, 2] = rng.uniform(0.7, 1.1, size=(n_env, cap))
    quat = rng.normal(size=(n_env, cap, 4))
    q[:, :, 3:7] = quat / np.linalg.norm(quat, axis=-1, keepdims=True)
    q[:, :, 7:] = rng.uniform(-0.6, 0.6, size=(n_env, cap, 69))
    rows = np.array([cap, 1, R], dtype=np.int32)
    rec.pred_qpos.copy_(dev(q))
    rec.rows.copy_(dev(rows))
    smpl = [MC.synthetic_model(50, 8), MC.synthetic_model(50, 9)]
    mesh = EO.SmplMesh(smpl)
    betas, gender = rng.normal(size=(n_env, 16)), np.array([1, 0, 1], dtype=np.int32)
    res = EO.mesh_metrics_of_record(mesh, rec, model, dev(betas), seq_gender=gender, want=("metrics", "zmin"), wait=True)
    assert res["bad"] == 0 and res["row_out"].shape == (n_env, cap, 4) and res["seq_means"].shape == (n_env, 4)
    pose_aa, trans, _ = EO.smpl_of_record(rec, model, wait=True)
    for e in range(n_env):
        T = int(rows[e])
        vert, _ = SM.lbs_numpy(smpl[gender[e]], pose_aa[e, :T].cpu().numpy(), betas[e, :10], trans[e, :T].cpu().numpy())
        assert np.abs(vert[:, :, 2]).min() > MC.FLOOR_MARGIN
        exp_rows, exp_means = SM.mesh_metrics_numpy(vert, 0.0)
        got = res["row_out"][e].cpu().numpy()
        np.testing.assert_allclose(got[:T, [0, 2, 3]], exp_rows[:, [0, 2, 3]], rtol=0, atol=MC.METRIC_ATOL)
        np.testing.assert_allclose(got[:T - 1, 1], exp_rows[:T - 1, 1], rtol=0, atol=MC.METRIC_ATOL)
        assert np.isnan(got[T:]).all() and np.isnan(got[T - 1, 1])
        np.testing.assert_allclose(res["seq_means"][e].cpu().numpy(), exp_means, rtol=0, atol=MC.METRIC_ATOL, equal_nan=True)
        np.testing.assert_allclose(res["zmin"][e, :T].cpu().numpy(), vert[:, :, 2].min(axis=1), rtol=0, atol=MC.VERT_ATOL)
    mesh.close()


def test_mesh_metrics_of_a_bank_match_the_host_functions():
    import os
    from uhc_amd import eval_ops as EO
    from uhc_amd import sim as S
    from uhc_amd.sim import load_asset_model
    from uhc_amd.smpllib.smpl_mujoco import qpos_to_smpl
    from uhc_amd.smpllib.torch_smpl_humanoid import Humanoid
    model = load_asset_model()
    z = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uhc_amd", "assets", "standing_neutral.npz"))
    rng = np.random.default_rng(9)
    lens = [1, R + 1, 4]
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    n = sum(lens)
    qpos = np.tile(z["qpos"], (n, 1))
    qpos[:, 7:] += rng.normal(scale=0.1, size=(n, qpos.shape[1] - 7))
    qpos[:, :2] += np.cumsum(rng.normal(scale=0.01, size=(n, 2)), axis=0)
    frames = S.expert_frames_device(torch.from_numpy(qpos), list(starts), [Humanoid(model=model)], device=torch.device("cuda", 0))
    smpl = [MC.synthetic_model(50, 8)]
    mesh = EO.SmplMesh(smpl)
    betas = rng.normal(size=(3, 10))
    res = EO.mesh_metrics_of_bank(mesh, frames, starts, lens, model, betas, wait=True)
    assert res["bad"] == 0 and res["row_out"].shape == (n, 4) and res["seq_means"].shape == (3, 4)
    for s, (g0, T) in enumerate(zip(starts, lens)):
        pose, trans = qpos_to_smpl(frames[g0:g0 + T, 0:76].cpu().numpy(), model)
        vert, _ = SM.lbs_numpy(smpl[0], pose.reshape(T, 72), betas[s], trans)
        assert np.abs(vert[:, :, 2]).min() > MC.FLOOR_MARGIN
        exp_rows, exp_means = SM.mesh_metrics_numpy(vert, 0.0)
        got = res["row_out"][g0:g0 + T].cpu().numpy()
        np.testing.assert_allclose(got[:, [0, 2, 3]], exp_rows[:, [0, 2, 3]], rtol=0, atol=MC.METRIC_ATOL)
        np.testing.assert_allclose(got[:T - 1, 1], exp_rows[:T - 1, 1], rtol=0, atol=MC.METRIC_ATOL)
        np.testing.assert_allclose(res["seq_means"][s].cpu().numpy(), exp_means, rtol=0, atol=MC.METRIC_ATOL, equal_nan=True)
    mesh.close()


def test_device_fix_height_is_the_host_computation_with_pose_blend_shapes(tmp_path):
    import pickle
    from uhc_amd.smpllib.smpl_robot import make_fix_height
    tabs = MC.synthetic_tables(50, 6)
    with open(tmp_path / "SMPL_MALE.pkl", "wb") as f:
        pickle.dump(tabs, f)
    provider = SM.MeshBodyProvider(str(tmp_path))
    fix = make_fix_height(provider, device=True)
    rng = np.random.default_rng(3)
    pose, betas, trans = MC.random_poses(rng, 6), rng.normal(size=16), rng.normal(size=(6, 3))
    out = fix(pose, betas, trans, np.array("male"))
    v0 = SM.lbs_numpy(provider.model(1), pose[:1], betas[:10], trans[:1])[0][0]
    want = trans.copy()
    want[:, 2] -= v0[:, 2].min()
    np.testing.assert_allclose(out, want, rtol=0, atol=MC.VERT_ATOL)
    assert np.array_equal(out[:, :2], trans[:, :2])
    # ... which is not the default's height: that one skins without the pose blend shapes
    host = make_fix_height(provider)(pose, betas, trans, "male")
    assert np.abs(host[0, 2] - out[0, 2]) > 1e-6
    with pytest.raises(Exception, match="Gender Not Supported"):
        fix(pose, betas, trans, "other")


def test_eval_seqs_scores_the_smpl_mesh_on_both_builds(tmp_path):
    import copy
    import pickle
    from tests.test_gpu_agent import _cfg
    from uhc_amd.agents import agent_dict
    from uhc_amd.data_loaders.dataset_amass_single import DatasetAMASSSingle
    from uhc_amd.data_loaders.synthetic import make_synthetic_amass
    torch.set_default_dtype(torch.float64)
    cfg = _cfg(tmp_path, n_env=2, batch=2 * 4)
    specs = dict(cfg.data_specs)
    specs["file_path"] = "synthetic"
    loader = DatasetAMASSSingle(specs, "train", pickle_data=make_synthetic_amass(2, seed=4, t_range=(12, 20)))
    agent = agent_dict[cfg.agent_name](cfg, torch.float64, torch.device("cuda", 0), data_loader=loader)
    agent.cfg.fail_safe = False
    smpl_dir = tmp_path / "smpl"
    smpl_dir.mkdir()
    for name, seed in (("SMPL_NEUTRAL", 1), ("SMPL_MALE", 2), ("SMPL_FEMALE", 3)):
        with open(smpl_dir / (name + ".pkl"), "wb") as f:
            pickle.dump(MC.synthetic_tables(50, seed), f)
    rs = agent.running_state.rs
    st = copy.deepcopy(rs.__getstate__())

    def passes():
        out = {}
        for build in ("host", "device"):
            rs._n = st["_n"]
            rs._M[...], rs._S[...] = st["_M"], st["_S"]
            rs._host_changed()
            agent.cfg.eval_build = build
            out[build] = agent.eval_seqs(list(loader.data_keys), loader)
        agent.cfg.eval_build = "host"
        return out

    assert agent.cfg.eval_mesh is False
    off = passes()
    agent.cfg.eval_mesh = str(smpl_dir)
    on = passes()
    four = ["pentration", "skate", "float", "contact"]
    for build in ("host", "device"):
        for k, res in on[build].items():
            assert list(res) == list(off[build][k]) + four, (build, list(res))
            for name, a in off[build][k].items():  # every other array: what it is without the key, to the bit
                assert np.array_equal(np.asarray(res[name]), np.asarray(a)), (build, k, name)
    for k, h in on["host"].items():
        d = on["device"][k]
        assert h["contact"].shape == d["contact"].shape == (h["pred"].shape[0],) and d["contact"].dtype == np.float64
        for name in four:
            print(k, name, "host", np.asarray(h[name]).ravel()[:3], "max |host - device| =", float(np.abs(np.asarray(h[name]) - np.asarray(d[name])).max()))
            np.testing.assert_allclose(d[name], h[name], rtol=0, atol=MC.METRIC_ATOL, err_msg=f"{k} {name}")
        assert np.ndim(d["pentration"]) == 0 and np.ndim(d["skate"]) == 0 and np.ndim(d["float"]) == 0
    agent.env.close()
