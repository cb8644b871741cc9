"""Inputs shared by tests/test_smpl_convert_cpu.py (the host build of uhc_smpl_convert.h) and tests/test_gpu_smpl_qpos.py (the kernel): the random poses, the
named edge cases and the properties of those inputs that make a 1e-9 comparison with `smpl_to_qpose` meaningful.  No test lives here.

Tolerance: 1e-9 absolute on every entry, the env layer's bar.  The Euler triple is ill-conditioned where cos Y -> 0 (Z and X turn about nearly the same axis): a
relative perturbation of 1e-15 of the quaternion moves an angle by at most 9.1e-13 where |cos Y| >= 1e-3, so the inputs are ASSERTED to stay there; the root
quaternion's sign flips at its branch boundaries, so the inputs are asserted to keep a margin of 1e-6 from them.  Nothing is excluded from a comparison."""
import numpy as np

TOL = 1e-9
N_RANDOM = 2048


def slot_of_joint(mj_model):
    """-> (smpl_2_mujoco, its inverse as int32): model slot m takes SMPL joint smpl_2_mujoco[m]"""
    from uhc_amd.smpllib.smpl_mujoco import smpl_to_model_table
    s2m = smpl_to_model_table(mj_model)
    inv = np.zeros(24, dtype=np.int32)
    inv[s2m] = np.arange(24)
    return s2m, inv


def random_poses():
    """2048 frames of large random rotation vectors (angles up to ~7.3 rad: beyond 2 pi) with random translations"""
    rng = np.random.default_rng(7)
    pose = rng.normal(scale=1.5, size=(N_RANDOM, 24, 3))
    trans = rng.normal(size=(N_RANDOM, 3))
    return pose.reshape(N_RANDOM, 72), trans


def assert_well_conditioned(pose):
    """the conditions under which host and device must agree to TOL, asserted on the inputs themselves (host side, scipy)"""
    from scipy.spatial.transform import Rotation as sRot
    rot = sRot.from_rotvec(np.asarray(pose).reshape(-1, 3))
    cos_y = np.cos(rot.as_euler("ZYX")[:, 1])
    assert (np.abs(cos_y) < 1e-3).sum() == 0, np.abs(cos_y).min()
    R = rot.as_matrix().reshape(-1, 24, 3, 3)[:, 0]
    m00, m11, m22 = R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]
    d2 = m22 < 1e-6
    # the boundaries a frame's branch depends on: m22 = 1e-6 always, then m00 = m11 (below it) or m00 = -m11 (above it)
    margin = np.minimum(np.abs(m22 - 1e-6), np.where(d2, np.abs(m00 - m11), np.abs(m00 + m11)))
    assert margin.min() > 1e-6, margin.min()
    branch = np.where(d2, np.where(m00 > m11, 0, 1), np.where(m00 < -m11, 2, 3))
    return np.bincount(branch, minlength=4), margin.min(), np.abs(cos_y).min()


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def edge_rotvecs():
    """name -> rotation vector.  None lies within 1e-6 of the 1e-7 lock threshold: the two lock cases sit AT lock (beta' of the order of 1e-16), everything else
    far from it."""
    from scipy.spatial.transform import Rotation as sRot
    u = _unit([1.0, -2.0, 0.5])
    exact = np.array([1e-3, 0.0, 0.0])  # |r| = 1e-3 exactly: the series' side of scipy's `<=`
    assert np.sqrt(exact @ exact) == 1e-3
    return {
        "zero": np.zeros(3),
        "1e-3 exactly": exact,
        "just below 1e-3": u * (1e-3 * (1 - 1e-9)),
        "just above 1e-3": u * (1e-3 * (1 + 1e-9)),
        "1e-8": u * 1e-8,
        "beyond 2 pi": u * 7.0,
        "lock +pi/2": sRot.from_euler("ZYX", (0.3, np.pi / 2, 0.2)).as_rotvec(),
        "lock -pi/2": sRot.from_euler("ZYX", (0.3, -np.pi / 2, 0.2)).as_rotvec(),
    }


def assert_away_from_the_lock_threshold(rotvecs):
    """no input near the 1e-7 threshold on beta' (or on |beta' - pi|): a case is either AT lock (below 1e-9, a hundredth of the threshold) or more than 1e-6
    beyond it, so the side it falls on cannot hinge on a last bit"""
    from scipy.spatial.transform import Rotation as sRot
    x, y, z, w = sRot.from_rotvec(np.asarray(rotvecs).reshape(-1, 3)).as_quat().T
    beta = 2 * np.arctan2(np.hypot(y + w, z - x), np.hypot(w - y, x + z))
    for b in (beta, np.abs(beta - np.pi)):
        assert ((b < 1e-9) | (b > 1e-6 + 1e-7)).all(), b


LOCK_EXPECT ={"lock +pi/2": (0.1, np.pi / 2), "lock -pi/2": (0.5, -np.pi / 2)}  # (Z, Y); X = 0 exactly
NEAR_LOCK = (0.1, np.pi / 2 - 1e-5, 0.4)  # not locked, ill-conditioned (cos Y = 1e-5): compared in rotation space only


def edge_poses():
    """One frame per edge case: the case's rotation vector on EVERY joint (so that it passes through the root's conversion and through each slot's),
    on top of a translation.  -> names, pose (n, 72), trans (n, 3)"""
    cases = edge_rotvecs()
    names = list(cases)
    assert_away_from_the_lock_threshold(np.stack([cases[k] for k in names] + [near_lock_pose()[0]]))
    pose =np.stack([np.tile(cases[k], 24) for k in names])
    trans = np.arange(3 * len(names), dtype=np.float64).reshape(-1, 3) * 0.1
    return names, pose, trans


def near_lock_pose():
    from scipy.spatial.transform import Rotation as sRot
    rv = sRot.from_euler("ZYX", NEAR_LOCK).as_rotvec()
    return rv, np.tile(rv, 24)[None]


def assert_rows_match_host(qpos, qpos_quat, pose, trans, mj_model, count_offset=True, names=None):
    """every entry of the 76-wide and / or 99-wide rows against smpl_to_qpose at TOL"""
    from uhc_amd.smpllib.smpl_mujoco import smpl_to_qpose
    for got, use_quat in ((qpos, False), (qpos_quat, True)):
        if got is None:
            continue
        want = smpl_to_qpose(pose, mj_model, trans=trans, count_offset=count_offset, use_quat=use_quat)
        assert got.shape == want.shape
        err = np.abs(got - want)
        assert np.isfinite(got).all()
        worst = np.unravel_index(np.argmax(err), err.shape)
        assert err.max() <= TOL, (use_quat, err.max(), worst, None if names is None else names[worst[0]])


def assert_lock_rows(qpos, names, s2m):
    """the two lock cases: X = 0 exactly and Z = 0.1 / 0.5 on every hinge triple of the row"""
    for name, (z, y) in LOCK_EXPECT.items():
        tri = qpos[names.index(name), 7:].reshape(23, 3)
        assert np.array_equal(tri[:, 2], np.zeros(23)), name
        np.testing.assert_allclose(tri[:, 0], z, atol=TOL, rtol=0, err_msg=name)
        np.testing.assert_allclose(tri[:, 1], y, atol=TOL, rtol=0, err_msg=name)


def assert_near_lock_row(qpos_row, rv):
    """the rotation rebuilt from each hinge triple is within TOL rad of the input rotation"""
    from scipy.spatial.transform import Rotation as sRot
    tri = qpos_row[7:].reshape(23, 3)
    assert np.abs(np.cos(tri[:, 1])).max() < 2e-5  # (ill-conditioned indeed, and not locked: X is not 0)
    assert np.abs(tri[:, 2]).min() > 0.1
    back = sRot.from_euler("ZYX", tri) * sRot.from_rotvec(rv).inv()
    assert back.magnitude().max() <= TOL, back.magnitude().max()
