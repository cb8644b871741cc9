"""Comparisons against the reference's own outputs, recorded by tools/gen_golden.py (g15_config_all, g16_boundary_helpers) where the
reference was importable: both sides once ran in the same process there; here the reference's side is the stored fixture."""
import json
import os
import sys
import tempfile

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _dec(v):
    if isinstance(v, dict):
        return np.asarray(v["__ndarray__"], dtype=float) if set(v) == {"__ndarray__"} else {k: _dec(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_dec(x) for x in v]
    return v


def _same(v, w):
    if isinstance(v, np.ndarray) or isinstance(w, np.ndarray):
        return np.array_equal(np.asarray(v, dtype=float), np.asarray(w, dtype=float), equal_nan=True)
    if isinstance(v, float) and np.isinf(v):
        return bool(np.isinf(w))
    return v == w


def test_config_equals_reference_on_every_shipped_config():
    """Every yml under the reference's config/ that the reference's own Config can load (85 of 115: the rest name model files it does
    not ship) gives the same attributes through uhc_amd's Config -- a yml written for the reference loads unchanged."""
    import uhc  # noqa: F401  -- this build's alias package: the comparison must survive it being imported first
    from uhc_amd.utils.config_utils.copycat_config import Config as MyConfig
    assert os.sep + "uhc_amd" + os.sep in os.path.realpath(MyConfig.__init__.__code__.co_filename)
    assert sys.modules["uhc"] is uhc
    recorded = json.loads(str(np.load(os.path.join(GOLD, "g15_config_all.npz"))["configs"]))
    assert len(recorded) > 100
    compared = 0
    for f, rec in sorted(recorded.items()):
        if rec["attrs"] is None:
            continue  # the config names a model file the reference does not ship
        mc = MyConfig(cfg_id=rec["cfg_id"], base_dir=tempfile.mkdtemp(), cfg_dict=json.loads(json.dumps(rec["yml"])))
        for k, v in rec["attrs"].items():
            v = _dec(v)
            assert hasattr(mc, k), (f, k)
            assert _same(v, getattr(mc, k)), (f, k, v, getattr(mc, k))
        compared += 1
    assert compared >= 80


def test_new_boundary_helpers_equal_the_references():
    """get_qvel_fd_new, quat_mul_vec_batch, quaternion_from_euler_batch ('rzyx'), qpos_to_smpl, in_hull: this build's functions against the
    reference's outputs on the same seeded inputs."""
    from scipy.spatial import ConvexHull
    g = np.load(os.path.join(GOLD, "g16_boundary_helpers.npz"))
    from uhc_amd.sim import load_asset_model
    from uhc_amd.smpllib.smpl_mujoco import qpos_to_smpl
    from uhc_amd.smpllib.smpl_robot import in_hull
    from uhc_amd.utils.math_utils import get_qvel_fd_new
    from uhc_amd.utils.transformation import quat_mul_vec_batch, quaternion_from_euler_batch
    model = load_asset_model()
    q0, q1, ang = g["q0"], g["q1"], g["ang"]
    np.testing.assert_allclose(get_qvel_fd_new(q0, q1, 1 / 30), g["qvel"], atol=1e-10)
    np.testing.assert_allclose(get_qvel_fd_new(q0, q1, 1 / 30, "heading"), g["qvel_heading"], atol=1e-10)
    np.testing.assert_allclose(quat_mul_vec_batch(g["qs"], g["vs"]), g["rot"], atol=1e-13)
    np.testing.assert_allclose(quaternion_from_euler_batch(ang[0], ang[1], ang[2], "rzyx"), g["eul"], atol=1e-13)
    np.testing.assert_array_equal(in_hull(ConvexHull(g["pts"]), g["queries"]), g["in_hull"])
    pose, trans = qpos_to_smpl(g["qpos"], model)
    np.testing.assert_allclose(pose, g["pose"], atol=1e-10)
    np.testing.assert_allclose(trans, g["trans"], atol=1e-13)
