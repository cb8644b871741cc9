"""Inputs shared by tests/test_smpl_pose_cpu.py (the host build of the way back in uhc_smpl_convert.h) and tests/test_gpu_qpos_smpl.py (the kernels): random qpos
rows, the named edge rows, and the properties of those inputs that make a 1e-9 comparison with `qpos_to_smpl` / `qpos_quat_to_smpl` meaningful.  No test lives here.

Tolerance: 1e-9 absolute on every output entry (smpl_convert_cases.TOL, the env layer's bar).  The rotation vector is discontinuous in two places only: at w = 0 it
jumps to its antipode (as_rotvec negates a quaternion with w < 0), and at an angle of 1e-3 scipy changes formula (harmless: the two agree to 1e-18 there, asserted
all the same).  The random rows are ASSERTED to stay clear of both; a 1e-15 relative perturbation of their angles moves scipy's rotation vector by 1.0e-14.  Nothing
is excluded from a comparison."""
import numpy as np

from tests.smpl_convert_cases import TOL, slot_of_joint  # noqa: F401  (re-exported: one bar, one table)

N_RANDOM = 2048
SENTINEL = -7.0


def random_rows(ball=False):
    """-> 2048 qpos rows: hinge rows (2048, 76), or ball-joint rows (2048, 99).  Hinge triples normal(scale=1.5) -- beyond +-pi on purpose, hinge angles are not
    wrapped --, quaternions normal(size=4) * uniform(0.5, 2) -- non-unit on purpose --, translations normal."""
    rng = np.random.default_rng(11)
    tri = rng.normal(scale=1.5, size=(N_RANDOM, 23, 3))
    root = rng.normal(size=(N_RANDOM, 4)) * rng.uniform(0.5, 2.0, size=(N_RANDOM, 1))
    trans = rng.normal(size=(N_RANDOM, 3))
    if not ball:
        return np.concatenate([trans, root, tri.reshape(N_RANDOM, 69)], axis=1)
    quats = rng.normal(size=(N_RANDOM, 23, 4)) * rng.uniform(0.5, 2.0, size=(N_RANDOM, 23, 1))
    return np.concatenate([trans, root, quats.reshape(N_RANDOM, 92)], axis=1)


def joint_quats(rows, ball=False):
    """every joint of every row as scipy holds it: (n_rows * 24, 4) unit quaternions (x, y, z, w), model order"""
    from scipy.spatial.transform import Rotation as sRot
    rows = np.asarray(rows)
    if ball:
        return sRot.from_quat(rows[:, 3:99].reshape(-1, 4)[:, [1, 2, 3, 0]]).as_quat()
    root = sRot.from_quat(rows[:, [4, 5, 6, 3]]).as_quat()
    tri = sRot.from_euler("ZYX", rows[:, 7:76].reshape(-1, 3)).as_quat().reshape(-1, 23, 4)
    return np.concatenate([root[:, None], tri], axis=1).reshape(-1, 4)


def assert_well_conditioned(rows, ball=False):
    """the conditions under which host and device must agree to TOL, asserted on the inputs themselves (host side, scipy) -> (min |w|, min and max angle)"""
    from scipy.spatial.transform import Rotation as sRot
    q = joint_quats(rows, ball)
    assert (np.abs(q[:, 3]) > 1e-6).all(), np.abs(q[:, 3]).min()  # at w = 0 the rotation vector jumps to its antipode
    angle = sRot.from_quat(q).magnitude()
    assert (np.abs(angle - 1e-3) > 1e-6).all()                   # the series threshold of as_rotvec
    return np.abs(q[:, 3]).min(), angle.min(), angle.max()


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _quat_wxyz(angle, axis=(1.0, -2.0, 0.5)):
    u = _unit(axis)
    return np.r_[np.cos(angle / 2), np.sin(angle / 2) * u]


EDGE_NAMES = ["identity", "1e-3 exactly", "just below 1e-3", "just above 1e-3", "1e-8", "pi - 1e-9", "w exactly 0", "w < 0", "triples beyond 2 pi", "non-unit root",
              "zero root", "NaN triple"]
BAD_NAMES = ("zero root", "NaN triple")


def edge_rows(ball=False):
    """One row per edge case, the case on EVERY joint: the root and -- ball-joint rows -- every joint hold the case's quaternion (w, x, y, z); the hinge triples of
    a hinge row hold the case's rotation as intrinsic ZYX angles where that is well conditioned (|w| > 1e-6, and not the two quaternion-only cases), the triple the
    case names, or zeros.  The last two rows are bad rows: NaN in every output, counted.  -> names, rows (n, 76 or 99)"""
    from scipy.spatial.transform import Rotation as sRot
    z = np.array([0.0, 0.0, 1.0])
    quat = {
        "identity": np.r_[1.0, 0.0, 0.0, 0.0],
        "1e-3 exactly": _quat_wxyz(1e-3, z),
        "just below 1e-3": _quat_wxyz(1e-3 * (1 - 1e-9)),
        "just above 1e-3": _quat_wxyz(1e-3 * (1 + 1e-9)),
        "1e-8": _quat_wxyz(1e-8),
        "pi - 1e-9": _quat_wxyz(np.pi - 1e-9),
        "w exactly 0": np.r_[0.0, _unit([0.6, -0.3, 0.2])],     # not negated: angle pi about +axis
        "w < 0": -_quat_wxyz(1.1),                                # negated by as_rotvec: the same rotation as angle 1.1
        "triples beyond 2 pi": _quat_wxyz(0.7),
        "non-unit root": 3.7 * _quat_wxyz(2.0),
        "zero root": np.zeros(4),
        "NaN triple": _quat_wxyz(0.4),
    }
    assert quat["pi - 1e-9"][0] > 0 and quat["w exactly 0"][0] == 0.0 and quat["w < 0"][0] < 0
    triple = {"triples beyond 2 pi": np.r_[7.0, -6.5, 9.0], "NaN triple": np.r_[0.1, np.nan, 0.2], "1e-3 exactly": np.r_[1e-3, 0.0, 0.0], "zero root": np.r_[0.3, 0.2, 0.1]}
    rows = []
    for k, name in enumerate(EDGE_NAMES):
        q = quat[name]
        trans = 0.1 * np.arange(3 * k, 3 * k + 3)
        if ball:
            joints = np.tile(q, 23)
            if name == "zero root":
                joints = np.tile(_quat_wxyz(0.5), 23)  # (only the root is zero: one bad joint spoils the row)
            if name == "NaN triple":
                joints[4 * 11 + 2] = np.nan            # (a ball-joint row has no triple: one NaN component of one joint)
        elif name in triple:
            joints = np.tile(triple[name], 23)
        elif abs(q[0]) / np.linalg.norm(q) > 1e-6 and name not in ("w < 0", "non-unit root"):
            joints = np.tile(sRot.from_quat(q[[1, 2, 3, 0]]).as_euler("ZYX"), 23)
        else:
            joints = np.zeros(69)
        rows.append(np.r_[trans, q, joints])
    return list(EDGE_NAMES), np.stack(rows)


def host_pose(rows, mj_model, ball=False, count_offset=True):
    """the host functions on rows of any width >= 76 / 99 -> (pose_aa (n, 72), trans (n, 3)); bad rows (scipy raises, or NaN comes out) are NaN throughout"""
    from uhc_amd.smpllib.smpl_mujoco import qpos_quat_to_smpl, qpos_to_smpl
    rows = np.asarray(rows, dtype=np.float64)
    f = qpos_quat_to_smpl if ball else qpos_to_smpl
    pose, trans = np.full((rows.shape[0], 72), np.nan), np.full((rows.shape[0], 3), np.nan)
    for r in range(rows.shape[0]):  # (row by row: scipy refuses a whole batch for one zero quaternion)
        try:
            with np.errstate(invalid="ignore"):
                p, t = f(rows[r:r + 1], mj_model)
        except ValueError:
            continue
        if np.isfinite(p).all():
            pose[r], trans[r] = p.reshape(72), t[0]
    if not count_offset:
        trans = trans + np.asarray(mj_model.body_pos)[1]
    return pose, trans


def host_pose_fast(rows, mj_model, ball=False):
    """the host functions on a whole batch without bad rows"""
    from uhc_amd.smpllib.smpl_mujoco import qpos_quat_to_smpl, qpos_to_smpl
    pose, trans = (qpos_quat_to_smpl if ball else qpos_to_smpl)(np.asarray(rows, dtype=np.float64), mj_model)
    return pose.reshape(-1, 72), trans


def host_6d(pose_aa, trans):
    """[trans | 24 x (column 0, column 1 of Rotation.as_matrix)] in float64: convert_aa_to_orth6d's layout"""
    from scipy.spatial.transform import Rotation as sRot
    pose_aa = np.asarray(pose_aa).reshape(-1, 72)
    R = np.full((pose_aa.shape[0] * 24, 3, 3), np.nan)
    ok = np.isfinite(pose_aa.reshape(-1, 3)).all(axis=1)
    R[ok] = sRot.from_rotvec(pose_aa.reshape(-1, 3)[ok]).as_matrix()
    d6 = np.concatenate([R[:, :, 0], R[:, :, 1]], axis=1).reshape(-1, 144)
    return np.concatenate([np.asarray(trans), d6], axis=1)


def assert_close(got, want, names=None, what=""):
    """every entry at TOL; NaN exactly where the reference is NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.argwhere(np.isnan(got) != np.isnan(want))[:4])
    err = np.nan_to_num(np.abs(got - want), nan=0.0)
    worst = np.unravel_index(np.argmax(err), err.shape)
    assert err.max() <= TOL, (what, err.max(), worst, None if names is None else names[worst[0]])
