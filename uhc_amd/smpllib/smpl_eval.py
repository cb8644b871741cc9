"""Imitation metrics (mirror of uhc/smpllib/smpl_eval.py:24-126): mpjpe, global mpjpe, Procrustes-aligned
mpjpe, velocity / acceleration error (all in mm), root transform distance, success.  Vectorised numpy."""
import numpy as np

from ..utils.transformation import quaternion_matrix


def p_mpjpe(predicted, target):
    """MPJPE after similarity (scale, rotation, translation) alignment per frame (smpl_eval.py:24-63)."""
    muX, muY = target.mean(axis=1, keepdims=True), predicted.mean(axis=1, keepdims=True)
    X0, Y0 = target - muX, predicted - muY
    normX = np.sqrt((X0 ** 2).sum(axis=(1, 2), keepdims=True))
    normY = np.sqrt((Y0 ** 2).sum(axis=(1, 2), keepdims=True))
    X0, Y0 = X0 / normX, Y0 / normY
    U, s, Vt = np.linalg.svd(np.matmul(X0.transpose(0, 2, 1), Y0))
    V = Vt.transpose(0, 2, 1)
    R = np.matmul(V, U.transpose(0, 2, 1))
    sign = np.sign(np.linalg.det(R))[:, None]
    V[:, :, -1] *= sign
    s[:, -1] *= sign.ravel()
    R = np.matmul(V, U.transpose(0, 2, 1))
    a = s.sum(axis=1)[:, None, None] * normX / normY
    t = muX - a * np.matmul(muY, R)
    return np.linalg.norm(a * np.matmul(predicted, R) + t - target, axis=-1)


def _root_matrices(qpos):
    out = np.stack([quaternion_matrix(q[3:7]) for q in qpos])
    out[:, :3, 3] = qpos[:, :3]
    return out


def compute_metrics(res, converter=None):
    """res: {"pred", "gt": (T, nq) qpos; "pred_jpos", "gt_jpos": (T, 3J) world joint positions; "fail_safe", "percent"}."""
    jp, jg = np.asarray(res["pred_jpos"]), np.asarray(res["gt_jpos"])
    T = np.asarray(res["pred"]).shape[0]
    jp, jg = jp.reshape(T, -1, 3), jg.reshape(T, -1, 3)
    Mp, Mg = _root_matrices(np.asarray(res["pred"])), _root_matrices(np.asarray(res["gt"]))
    err = np.eye(4)[None] - np.matmul(Mp, np.linalg.inv(Mg))
    out = {"root_dist": np.sqrt((err ** 2).sum(axis=(1, 2))) / T * 1000}
    vel = np.linalg.norm((jg[1:] - jg[:-1]) - (jp[1:] - jp[:-1]), axis=2)  # argument order of the reference: (pred, gt) swapped is symmetric
    acc = np.linalg.norm((jg[:-2] - 2 * jg[1:-1] + jg[2:]) - (jp[:-2] - 2 * jp[1:-1] + jp[2:]), axis=2)
    out["vel_dist"] = vel.mean(axis=-1) * 1000
    out["accel_dist"] = acc.mean(axis=-1) * 1000
    out["mpjpe_g"] = np.linalg.norm(jp - jg, axis=2).mean(axis=-1) * 1000
    root = 0 if jp.shape[1] == 24 else 7
    jp0, jg0 = jp - jp[:, root:root + 1], jg - jg[:, root:root + 1]
    out["pa_mpjpe"] = p_mpjpe(jp0, jg0).mean(axis=-1) * 1000
    out["mpjpe"] = np.linalg.norm(jp0 - jg0, axis=2).mean(axis=-1) * 1000
    out["succ"] = np.array([(not res["fail_safe"]) and res["percent"] == 1])
    if "pred_vertices" in res:  # smpl_eval.py:113-121: the two scalars, under the reference's spelling; the vertices do not stay in the result
        info = {"floor_z": 0}
        vert = np.asarray(res["pred_vertices"])
        out["pentration"] = np.mean(compute_penetration(vert, info))
        out["skate"] = np.mean(compute_skate(vert, info))
        out["float"] = np.mean(compute_float(vert, info))  # (ours: the counterpart that makes "penetration 0" readable)
        out["contact"] = compute_contact(vert, info)
        for k in ("pred_vertices", "gt_vertices", "gt_joints", "pred_joints"):
            res.pop(k, None)
    return out


# ---- contact quality (smpl_eval.py:125-149).  The reference scores SMPL surface vertices, which need the licensed SMPL files; this build scores the
# convex-hull vertices every compiled model carries (hull_vertices) -- a DEVIATION --, and adds `float`.  vert: (T, V, 3) world vertices, float64.
def compute_penetration(vert, info):
    """Per frame, in mm: how deep the vertices below the floor lie on average (0 when none does; strictly below, as the reference)."""
    h = np.asarray(vert, dtype=np.float64)[:, :, 2] - info["floor_z"]
    out = []
    for hz in h:
        under = hz < 0
        out.append(-hz[under].mean() * 1000 if under.any() else 0.0)
    return out


def compute_skate(vert, info):
    """Per pair of consecutive frames, in mm: how far the vertices that touch the floor in both (z <= floor_z) slide over it on average."""
    vert = np.asarray(vert, dtype=np.float64)
    touch = vert[:, :, 2] - info["floor_z"] <= 0
    out = []
    for t in range(vert.shape[0] - 1):
        both = touch[t] & touch[t + 1]
        d = vert[t + 1, both, :2] - vert[t, both, :2]
        out.append(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).mean() * 1000 if both.any() else 0.0)
    return out


def compute_float(vert, info):
    """Per frame, in mm: the height of the lowest vertex when every vertex lies above the floor, else 0.  (Not in the reference.)"""
    h = np.asarray(vert, dtype=np.float64)[:, :, 2] - info["floor_z"]
    return [hz.min() * 1000 if (hz > 0).all() else 0.0 for hz in h]


def compute_contact(vert, info):
    """Per frame: the number of vertices with z <= floor_z, as float64.  (Not in the reference.)"""
    return (np.asarray(vert, dtype=np.float64)[:, :, 2] - info["floor_z"] <= 0).sum(axis=1).astype(np.float64)


def surface_tables(model, body_lim=None):
    """The hull vertices of the humanoid's bodies 1 .. body_lim - 1 (default: all bodies) of a compiled model, in geom order: (vert (V, 3) in the body
    frame, vert_body (V,) int32 with body 1 as 0, vert_radius (V,): geom_size[0] of sphere and capsule cores, 0 of mesh hulls)."""
    from ..model.mjcf import geom_radius
    body_lim = int(model.nbody if body_lim is None else body_lim)
    rad = geom_radius(model)
    vert, body, radius = [], [], []
    for g in range(model.ngeom):
        b, a, n = int(model.geom_bodyid[g]), int(model.geom_vertadr[g]), int(model.geom_vertnum[g])
        if n <= 0 or a < 0 or not 1 <= b < body_lim:
            continue
        vert.append(np.asarray(model.mesh_vert[a:a + n], dtype=np.float64))
        body.append(np.full(n, b - 1, dtype=np.int32))
        radius.append(np.full(n, rad[g], dtype=np.float64))
    if not vert:
        raise ValueError("surface_tables: the model's humanoid bodies own no hull vertex")
    return np.concatenate(vert), np.concatenate(body), np.concatenate(radius)


def hull_vertices(model, xpos, xquat, body_lim=None):
    """World hull vertices of a motion: xpos (T, B, 3), xquat (T, B, 4) (w, x, y, z) of the bodies 1 .. B of `model` (or a surface_tables() triple) ->
    (T, V, 3), w = xpos[b] + R(xquat[b]) v with z lowered by the vertex's radius: the lowest point of a rounded hull under its core vertex.  R divides by
    |q|^2 (the identity below 4 eps) and every product and sum is rounded on its own, in the order of uhc_amd/csrc/uhc_surface_math.h."""
    vert, vb, vr = model if isinstance(model, tuple) else surface_tables(model, body_lim)
    xpos, xquat = np.asarray(xpos, dtype=np.float64), np.asarray(xquat, dtype=np.float64)
    T = xpos.shape[0]
    xpos, xquat = xpos.reshape(T, -1, 3), xquat.reshape(T, -1, 4)
    w, x, y, z = (xquat[:, :, k] for k in range(4))
    n = w * w + x * x + y * y + z * z
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(n < 4.0 * np.finfo(np.float64).eps, 0.0, 2.0 / n)
    R = [1.0 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w),
         s * (x * y + z * w), 1.0 - s * (x * x + z * z), s * (y * z - x * w),
         s * (x * z - y * w), s * (y * z + x * w), 1.0 - s * (x * x + y * y)]
    R = [r[:, vb] for r in R]  # (T, V)
    p = xpos[:, vb]
    v0, v1, v2 = vert[None, :, 0], vert[None, :, 1], vert[None, :, 2]
    out = np.empty((T, vert.shape[0], 3))
    for i in range(3):
        out[:, :, i] = p[:, :, i] + ((R[3 * i] * v0 + R[3 * i + 1] * v1) + R[3 * i + 2] * v2)
    out[:, :, 2] = out[:, :, 2] - vr[None]
    return out
