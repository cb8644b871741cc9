"""MJCF(+binary STL) -> flat rigid-body model arrays (host-side model compiler).

Replaces what the reference obtains from ``mujoco_py.load_model_from_xml``
(reference: uhc/khrylib/rl/envs/common/mujoco_env.py:18,34 and
uhc/envs/humanoid_im.py:1441-1454) for the MJCF subset the SMPL humanoid
models use (reference fixtures: assets/mujoco_models/humanoid_smpl_neutral_mesh.xml,
assets/mujoco_models/template/humanoid_template.xml, test.xml):

  compiler(angle, coordinate, inertiafromgeom) / default(joint, geom, motor)
  option(timestep, gravity, iterations, tolerance) / asset(mesh file=)
  worldbody -> nested body(name,pos,quat) { joint(free|ball|slide|hinge; stiffness, springref, frictionloss, damping, armature), geom(plane|mesh|box|sphere|capsule [size + pos/quat, or fromto]) }
  contact/exclude(body1, body2) / actuator/motor(joint, gear)

MuJoCo 2.1.0 itself is not available to this build; every
convention taken from MuJoCo is tagged [MJ-ext].

The output is a ``Model`` of numpy arrays (float64 / int32) that the C-ABI
(include/uhc_amd.h: ``UhcModelDesc``) consumes verbatim.
"""
from __future__ import annotations

import os
import struct
import xml.etree.ElementTree as ET
from dataclasses import dataclass, field, fields
from typing import Dict, List, Optional

import numpy as np

JNT_FREE, JNT_BALL, JNT_SLIDE, JNT_HINGE = 0, 1, 2, 3  # [MJ-ext] mjtJoint order
GEOM_PLANE, GEOM_SPHERE, GEOM_CAPSULE, GEOM_BOX, GEOM_MESH = 0, 2, 3, 6, 7  # [MJ-ext] mjtGeom values
# Geoms that collide as convex hulls: meshes, and the ROUNDED hulls -- a sphere is one vertex, a capsule the two end points of its segment, each pushed out by
# geom_size[0] (the radius) along the query direction.  They share the mesh geoms' vertex tables (geom_vertadr / geom_vertnum / mesh_vert / mesh_adj).
HULL_TYPES = (GEOM_MESH, GEOM_SPHERE, GEOM_CAPSULE)


def geom_radius(m: "Model") -> np.ndarray:
    """Inflation radius of every geom's hull: geom_size[0] of spheres and capsules, 0 for meshes (whose `size` MuJoCo ignores) and everything else."""
    t = np.asarray(m.geom_type)
    return np.where((t == GEOM_SPHERE) | (t == GEOM_CAPSULE), np.asarray(m.geom_size)[:, 0], 0.0)

MINVAL = 1e-15  # [MJ-ext] mjMINVAL


# --------------------------------------------------------------------------- #
# small quaternion helpers (w, x, y, z)
# --------------------------------------------------------------------------- #
def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([
        aw * bw - ax * bx - ay * by - az * bz,
        aw * bx + ax * bw + ay * bz - az * by,
        aw * by - ax * bz + ay * bw + az * bx,
        aw * bz + ax * by - ay * bx + az * bw,
    ])


def quat_conj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


def quat_to_mat(q):
    w, x, y, z = q
    return np.array([
        [w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
        [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
        [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z],
    ])


def mat_to_quat(R):
    """Rotation matrix -> unit quaternion (w>=0 branch by largest pivot)."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
        q = np.zeros(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    q /= np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    return q


# --------------------------------------------------------------------------- #
# meshes
# --------------------------------------------------------------------------- #
def load_binary_stl(path: str) -> np.ndarray:
    """Binary STL -> (ntri, 3, 3) float64 triangle soup (file floats are f32)."""
    with open(path, "rb") as f:
        data = f.read()
    (ntri,) = struct.unpack("<I", data[80:84])
    if len(data) < 84 + 50 * ntri:
        raise ValueError(f"{path}: truncated binary STL")
    rec = np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")])
    arr = np.frombuffer(data, dtype=rec, count=ntri, offset=84)
    return arr["v"].astype(np.float64)


def write_binary_stl(path: str, tris: np.ndarray) -> None:
    tris = np.asarray(tris, dtype=np.float32)
    rec = np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")])
    arr = np.zeros(len(tris), dtype=rec)
    arr["v"] = tris
    with open(path, "wb") as f:
        f.write(b"uhc_amd stl".ljust(80, b" "))
        f.write(struct.pack("<I", len(tris)))
        f.write(arr.tobytes())


def weld(tris: np.ndarray):
    """Triangle soup -> (unique verts (nv,3), faces (ntri,3) int) keeping first-seen order."""
    flat = tris.reshape(-1, 3)
    seen: Dict[bytes, int] = {}
    verts: List[np.ndarray] = []
    idx = np.empty(len(flat), dtype=np.int32)
    for i, v in enumerate(flat):
        key = v.tobytes()
        j = seen.get(key)
        if j is None:
            j = len(verts)
            seen[key] = j
            verts.append(v)
        idx[i] = j
    return np.array(verts), idx.reshape(-1, 3)


def polyhedron_mass_properties(verts: np.ndarray, faces: np.ndarray):
    """Exact volume, centre of mass and unit-density inertia (about the COM) of a
    closed triangulated surface, by signed tetrahedra against a reference point
    inside the mesh.  [MJ-ext] MuJoCo 2.1 (user_mesh.cc, mjCMesh::Process) uses the
    same decomposition around the area-weighted face centroid; the result for a
    closed surface is unique, so the two agree up to rounding."""
    ref = verts.mean(axis=0)
    a = verts[faces[:, 0]] - ref
    b = verts[faces[:, 1]] - ref
    c = verts[faces[:, 2]] - ref
    vol6 = np.einsum("ij,ij->i", a, np.cross(b, c))
    if vol6.sum() < 0:  # inward-facing winding
        vol6 = -vol6
    vol = vol6.sum() / 6.0
    com_rel = (vol6[:, None] * (a + b + c)).sum(axis=0) / (24.0 * vol)
    # second moments  integral x_i x_j dV over each tetra (0,a,b,c)
    # = vol6/120 * ( sum_p p_i p_j + (sum_p p_i)(sum_p p_j) ),  p in {a,b,c}
    s = a + b + c
    P = (np.einsum("ni,nj->nij", a, a) + np.einsum("ni,nj->nij", b, b)
         + np.einsum("ni,nj->nij", c, c) + np.einsum("ni,nj->nij", s, s))
    C = (vol6[:, None, None] * P).sum(axis=0) / 120.0  # about ref
    C -= vol * np.outer(com_rel, com_rel)  # about the COM
    inertia = np.trace(C) * np.eye(3) - C
    return vol, ref + com_rel, inertia


def hull_adjacency(nvert: int, faces: np.ndarray):
    """CSR vertex adjacency of a triangulated convex hull (edge graph). [MJ-ext] MuJoCo
    builds the same kind of graph from qhull output for hill-climbing support queries
    and for the plane-mesh multi-contact rule."""
    nbr: List[List[int]] = [[] for _ in range(nvert)]
    for f in faces:
        for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            if b not in nbr[a]:
                nbr[a].append(int(b))
            if a not in nbr[b]:
                nbr[b].append(int(a))
    adr = np.zeros(nvert + 1, dtype=np.int32)
    for i in range(nvert):
        adr[i + 1] = adr[i] + len(nbr[i])
    idx = np.array([j for l in nbr for j in l], dtype=np.int32)
    return adr, idx


# --------------------------------------------------------------------------- #
# the compiled model
# --------------------------------------------------------------------------- #
@dataclass
class Model:
    # sizes
    nq: int = 0
    nv: int = 0
    nu: int = 0
    nbody: int = 0
    njnt: int = 0
    ngeom: int = 0
    nmeshvert: int = 0
    nmeshadj: int = 0
    nexclude: int = 0
    # options
    timestep: float = 0.002
    gravity: np.ndarray = field(default_factory=lambda: np.array([0.0, 0.0, -9.81]))
    iterations: int = 100
    solver: int = 0  # 0: PGS sweeps (MuJoCo's mj_solPGS), 1: exact active-set solve of the same QP (include/uhc_amd.h)
    tolerance: float = 1e-8
    meaninertia: float = 1.0
    plane_mesh_maxcon: int = 4
    # names
    body_names: List[str] = field(default_factory=list)
    joint_names: List[str] = field(default_factory=list)
    geom_names: List[str] = field(default_factory=list)
    actuator_names: List[str] = field(default_factory=list)
    # bodies
    body_parentid: np.ndarray = None
    body_jntadr: np.ndarray = None
    body_jntnum: np.ndarray = None
    body_dofadr: np.ndarray = None
    body_dofnum: np.ndarray = None
    body_pos: np.ndarray = None
    body_quat: np.ndarray = None
    body_ipos: np.ndarray = None
    body_iquat: np.ndarray = None
    body_mass: np.ndarray = None
    body_inertia: np.ndarray = None
    body_invweight0: np.ndarray = None
    # joints
    jnt_type: np.ndarray = None
    jnt_bodyid: np.ndarray = None
    jnt_qposadr: np.ndarray = None
    jnt_dofadr: np.ndarray = None
    jnt_pos: np.ndarray = None
    jnt_axis: np.ndarray = None
    jnt_limited: np.ndarray = None
    jnt_range: np.ndarray = None
    jnt_stiffness: np.ndarray = None
    jnt_margin: np.ndarray = None
    qpos0: np.ndarray = None
    qpos_spring: np.ndarray = None
    # dofs
    dof_bodyid: np.ndarray = None
    dof_jntid: np.ndarray = None
    dof_parentid: np.ndarray = None
    dof_madr: np.ndarray = None
    dof_armature: np.ndarray = None
    dof_damping: np.ndarray = None
    dof_frictionloss: np.ndarray = None
    dof_invweight0: np.ndarray = None
    # geoms
    geom_type: np.ndarray = None
    geom_bodyid: np.ndarray = None
    geom_contype: np.ndarray = None
    geom_conaffinity: np.ndarray = None
    geom_condim: np.ndarray = None
    geom_pos: np.ndarray = None
    geom_quat: np.ndarray = None
    geom_size: np.ndarray = None
    geom_friction: np.ndarray = None
    geom_margin: np.ndarray = None
    geom_gap: np.ndarray = None
    geom_solref: np.ndarray = None
    geom_solimp: np.ndarray = None
    geom_rbound: np.ndarray = None
    geom_center: np.ndarray = None  # bounding-sphere centre in body frame
    geom_vertadr: np.ndarray = None
    geom_vertnum: np.ndarray = None
    mesh_vert: np.ndarray = None  # (nmeshvert,3) in BODY frame
    mesh_adjadr: np.ndarray = None  # (nmeshvert+1,) CSR, global vertex ids
    mesh_adj: np.ndarray = None
    # contact excludes (body pairs)
    exclude_pair: np.ndarray = None
    # actuators (motors on joints)
    actuator_dofid: np.ndarray = None
    actuator_gear: np.ndarray = None
    actuator_ctrlrange: np.ndarray = None

    @property
    def nM(self) -> int:
        return int(self.dof_madr[-1])

    # ---- convenience ----
    def body_id(self, name: str) -> int:
        return self.body_names.index(name)

    @property
    def _body_name2id(self) -> Dict[str, int]:
        return {n: i for i, n in enumerate(self.body_names)}

    def to_npz_dict(self) -> Dict[str, np.ndarray]:
        out = {}
        for f in fields(self):
            v = getattr(self, f.name)
            if isinstance(v, list):
                out[f.name] = np.array(v, dtype=object if not v else "U")
            elif isinstance(v, np.ndarray):
                out[f.name] = v
            else:
                out[f.name] = np.array(v)
        return out

    def save(self, path: str) -> None:
        np.savez_compressed(path, **self.to_npz_dict())

    @staticmethod
    def load(path: str) -> "Model":
        z = np.load(path, allow_pickle=False)
        m = Model()
        for f in fields(Model):
            if f.name not in z.files:
                continue
            v = z[f.name]
            cur = getattr(m, f.name)
            if isinstance(cur, list):
                setattr(m, f.name, [str(s) for s in v.tolist()])
            elif isinstance(cur, (int,)) and not isinstance(cur, bool) and v.shape == ():
                setattr(m, f.name, int(v))
            elif isinstance(cur, float) and v.shape == ():
                setattr(m, f.name, float(v))
            else:
                setattr(m, f.name, v)
        return m

    def copy(self) -> "Model":
        m = Model()
        for f in fields(Model):
            v = getattr(self, f.name)
            setattr(m, f.name, v.copy() if isinstance(v, np.ndarray) else (list(v) if isinstance(v, list) else v))
        return m


# --------------------------------------------------------------------------- #
# XML helpers
# --------------------------------------------------------------------------- #
def _floats(s: Optional[str], n: Optional[int] = None, default=None):
    if s is None:
        return None if default is None else np.array(default, dtype=np.float64)
    v = np.array([float(x) for x in s.split()], dtype=np.float64)
    if n is not None and len(v) != n:
        if len(v) < n and default is not None:  # partial spec, fill from default
            d = np.array(default, dtype=np.float64)
            d[: len(v)] = v
            return d
        raise ValueError(f"expected {n} numbers, got '{s}'")
    return v


def _bool(s: Optional[str], default: bool) -> bool:
    if s is None:
        return default
    return s.strip().lower() == "true"


class _Defaults:
    def __init__(self, root):
        self.joint: Dict[str, str] = {}
        self.geom: Dict[str, str] = {}
        self.motor: Dict[str, str] = {}
        d = root.find("default")
        if d is not None:
            for tag, store in (("joint", self.joint), ("geom", self.geom), ("motor", self.motor)):
                e = d.find(tag)
                if e is not None:
                    store.update(e.attrib)

    def get(self, kind: str, elem, key: str, fallback=None):
        v = elem.attrib.get(key)
        if v is not None:
            return v
        v = getattr(self, kind).get(key)
        return fallback if v is None else v


# --------------------------------------------------------------------------- #
# numpy kinematics + CRBA at a given qpos (needed at compile time for the
# constants MuJoCo's mj_setConst derives at qpos0: dof_invweight0,
# body_invweight0, stat.meaninertia [MJ-ext])
# --------------------------------------------------------------------------- #
def _z_to_quat(vec):
    """[MJ-ext] mjuu_z2quat: the rotation that takes the z axis onto `vec` (about z x vec)."""
    v = np.asarray(vec, dtype=np.float64)
    v = v / np.linalg.norm(v)
    ax = np.cross([0.0, 0.0, 1.0], v)
    sn = np.linalg.norm(ax)
    if sn < 1e-10:
        return np.array([1.0, 0, 0, 0]) if v[2] > 0 else np.array([0.0, 1.0, 0, 0])
    ang = np.arctan2(sn, v[2])
    return np.r_[np.cos(0.5 * ang), np.sin(0.5 * ang) * ax / sn]


def _axis_angle_quat(axis, angle):
    s = np.sin(angle * 0.5)
    return np.array([np.cos(angle * 0.5), axis[0] * s, axis[1] * s, axis[2] * s])


def kinematics_np(m: Model, qpos: np.ndarray):
    """World poses of bodies, joint anchors/axes (same recursion as [MJ-ext] mj_kinematics)."""
    xpos = np.zeros((m.nbody, 3))
    xquat = np.zeros((m.nbody, 4))
    xquat[0, 0] = 1.0
    xanchor = np.zeros((m.njnt, 3))
    xaxis = np.zeros((m.njnt, 3))
    for b in range(1, m.nbody):
        p = m.body_parentid[b]
        ja, jn = m.body_jntadr[b], m.body_jntnum[b]
        if jn == 1 and m.jnt_type[ja] == JNT_FREE:
            qa = m.jnt_qposadr[ja]
            pos = qpos[qa:qa + 3].copy()
            quat = qpos[qa + 3:qa + 7] / np.linalg.norm(qpos[qa + 3:qa + 7])
            xanchor[ja] = pos
            xaxis[ja] = [0, 0, 1]
        else:
            Rp = quat_to_mat(xquat[p])
            pos = xpos[p] + Rp @ m.body_pos[b]
            quat = quat_mul(xquat[p], m.body_quat[b])
            for j in range(ja, ja + jn):
                R = quat_to_mat(quat)
                xanchor[j] = pos + R @ m.jnt_pos[j]
                xaxis[j] = R @ m.jnt_axis[j]
                qa = m.jnt_qposadr[j]
                t = m.jnt_type[j]
                if t == JNT_HINGE:
                    quat = quat_mul(quat, _axis_angle_quat(m.jnt_axis[j], qpos[qa] - m.qpos0[qa]))
                elif t == JNT_BALL:
                    qb = qpos[qa:qa + 4] / np.linalg.norm(qpos[qa:qa + 4])
                    quat = quat_mul(quat, qb)
                elif t == JNT_SLIDE:
                    pos = pos + xaxis[j] * (qpos[qa] - m.qpos0[qa])
                    continue
                pos = xanchor[j] - quat_to_mat(quat) @ m.jnt_pos[j]
        quat = quat / np.linalg.norm(quat)
        xpos[b], xquat[b] = pos, quat
    return xpos, xquat, xanchor, xaxis


def dof_motion_axes_np(m: Model, xpos, xquat, xanchor, xaxis):
    """Per dof: (angular axis w, a point on the axis) in world frame; translational dofs have w=0
    and the direction stored separately."""
    w = np.zeros((m.nv, 3))
    lin = np.zeros((m.nv, 3))
    pt = np.zeros((m.nv, 3))
    for j in range(m.njnt):
        d = m.jnt_dofadr[j]
        b = m.jnt_bodyid[j]
        t = m.jnt_type[j]
        if t == JNT_FREE:
            lin[d:d + 3] = np.eye(3)
            R = quat_to_mat(xquat[b])
            for k in range(3):
                w[d + 3 + k] = R[:, k]
                pt[d + 3 + k] = xpos[b]
        elif t == JNT_BALL:
            R = quat_to_mat(xquat[b])
            for k in range(3):
                w[d + k] = R[:, k]
                pt[d + k] = xanchor[j]
        elif t == JNT_HINGE:
            w[d] = xaxis[j]
            pt[d] = xanchor[j]
        elif t == JNT_SLIDE:
            lin[d] = xaxis[j]
    return w, lin, pt


def point_jacobian_np(m: Model, w, lin, pt, body: int, point: np.ndarray):
    """(jacp 3xnv, jacr 3xnv) of a world point rigidly attached to ``body``."""
    jacp = np.zeros((3, m.nv))
    jacr = np.zeros((3, m.nv))
    b = body
    while b > 0:
        for d in range(m.body_dofadr[b], m.body_dofadr[b] + m.body_dofnum[b]):
            jacr[:, d] = w[d]
            jacp[:, d] = lin[d] + np.cross(w[d], point - pt[d])
        b = m.body_parentid[b]
    return jacp, jacr


def mass_matrix_np(m: Model, qpos: np.ndarray) -> np.ndarray:
    """Dense joint-space inertia (CRBA result + armature) via M = sum_b J_b^T I_b J_b."""
    xpos, xquat, xanchor, xaxis = kinematics_np(m, qpos)
    w, lin, pt = dof_motion_axes_np(m, xpos, xquat, xanchor, xaxis)
    M = np.zeros((m.nv, m.nv))
    for b in range(1, m.nbody):
        R = quat_to_mat(xquat[b])
        com = xpos[b] + R @ m.body_ipos[b]
        Ri = R @ quat_to_mat(m.body_iquat[b])
        I = Ri @ np.diag(m.body_inertia[b]) @ Ri.T
        jp, jr = point_jacobian_np(m, w, lin, pt, b, com)
        M += m.body_mass[b] * jp.T @ jp + jr.T @ I @ jr
    M += np.diag(m.dof_armature)
    return M


def set_const(m: Model) -> None:
    """[MJ-ext] mj_setConst restatement: dof_invweight0, body_invweight0, meaninertia at qpos0."""
    M = mass_matrix_np(m, m.qpos0)
    Minv = np.linalg.inv(M)
    m.meaninertia = float(np.trace(M) / max(1, m.nv))
    m.dof_invweight0 = np.zeros(m.nv)
    for j in range(m.njnt):
        d = m.jnt_dofadr[j]
        t = m.jnt_type[j]
        if t == JNT_FREE:
            m.dof_invweight0[d:d + 3] = np.mean(np.diag(Minv)[d:d + 3])
            m.dof_invweight0[d + 3:d + 6] = np.mean(np.diag(Minv)[d + 3:d + 6])
        elif t == JNT_BALL:
            m.dof_invweight0[d:d + 3] = np.mean(np.diag(Minv)[d:d + 3])
        else:
            m.dof_invweight0[d] = Minv[d, d]
    xpos, xquat, xanchor, xaxis = kinematics_np(m, m.qpos0)
    w, lin, pt = dof_motion_axes_np(m, xpos, xquat, xanchor, xaxis)
    m.body_invweight0 = np.zeros((m.nbody, 2))
    for b in range(1, m.nbody):
        com = xpos[b] + quat_to_mat(xquat[b]) @ m.body_ipos[b]
        jp, jr = point_jacobian_np(m, w, lin, pt, b, com)
        m.body_invweight0[b, 0] = max(MINVAL, np.trace(jp @ Minv @ jp.T) / 3.0)
        m.body_invweight0[b, 1] = max(MINVAL, np.trace(jr @ Minv @ jr.T) / 3.0)


# --------------------------------------------------------------------------- #
# compiler
# --------------------------------------------------------------------------- #
DEFAULT_SOLREF = (0.02, 1.0)  # [MJ-ext]
DEFAULT_SOLIMP = (0.9, 0.95, 0.001, 0.5, 2.0)  # [MJ-ext]
DEFAULT_FRICTION = (1.0, 0.005, 0.0001)  # [MJ-ext]
DEFAULT_DENSITY = 1000.0  # [MJ-ext]


def compile_mjcf(xml: str, asset_dir: str = ".", meshes: Optional[Dict[str, np.ndarray]] = None) -> Model:
    """Compile an MJCF string.  ``meshes`` optionally maps mesh name -> (ntri,3,3) triangles
    (bypasses file loading; used for per-env scaled bodies and tests)."""
    root = ET.fromstring(xml)
    comp = root.find("compiler")
    comp = comp.attrib if comp is not None else {}
    degree = comp.get("angle", "degree") == "degree"
    global_coord = comp.get("coordinate", "local") == "global"
    dfl = _Defaults(root)

    m = Model()
    opt = root.find("option")
    if opt is not None:
        m.timestep = float(opt.attrib.get("timestep", m.timestep))
        if "gravity" in opt.attrib:
            m.gravity = _floats(opt.attrib["gravity"], 3)
        m.iterations = int(opt.attrib.get("iterations", m.iterations))
        m.tolerance = float(opt.attrib.get("tolerance", m.tolerance))

    # ---- mesh assets ----
    mesh_tris: Dict[str, np.ndarray] = dict(meshes or {})
    asset = root.find("asset")
    if asset is not None:
        for me in asset.findall("mesh"):
            f = me.attrib.get("file")
            name = me.attrib.get("name") or os.path.splitext(os.path.basename(f))[0]
            if name in mesh_tris:
                continue
            if f is None:  # inline vertices (what export_mjcf writes): the mesh is their convex hull [MJ-ext]
                from .shapes import hull_triangles
                tri = hull_triangles(_floats(me.attrib["vertex"]).reshape(-1, 3))
            else:
                tri = load_binary_stl(os.path.join(asset_dir, f))
            if "scale" in me.attrib:
                tri = tri * _floats(me.attrib["scale"], 3)
            mesh_tris[name] = tri

    # ---- walk the body tree (MJCF order == depth-first == MuJoCo body ids) ----
    bodies = [dict(name="world", parent=0, gpos=np.zeros(3), gquat=np.array([1.0, 0, 0, 0]), joints=[], geoms=[])]

    def parse_geom(e, bid):
        g = dict(body=bid, name=e.attrib.get("name", ""))
        t = dfl.get("geom", e, "type", "sphere")
        g["type"] = {"plane": GEOM_PLANE, "sphere": GEOM_SPHERE, "capsule": GEOM_CAPSULE, "box": GEOM_BOX, "mesh": GEOM_MESH}[t]
        g["mesh"] = e.attrib.get("mesh")
        g["pos"] = _floats(e.attrib.get("pos"), 3, [0, 0, 0])
        g["quat"] = _floats(e.attrib.get("quat"), 4, [1, 0, 0, 0])
        sz = _floats(dfl.get("geom", e, "size"))
        sz = np.zeros(0) if sz is None else np.atleast_1d(sz)
        g["size"] = np.r_[sz, np.zeros(3)][:3]
        if "fromto" in e.attrib:  # [MJ-ext] capsule between two points: pos = their middle, z axis along the segment, size = (radius, half length)
            if g["type"] != GEOM_CAPSULE:
                raise ValueError("fromto is supported for capsules only")
            ft = _floats(e.attrib["fromto"], 6)
            d = ft[3:] - ft[:3]
            hl = 0.5 * np.linalg.norm(d)
            if hl < MINVAL:
                raise ValueError("capsule fromto: the two points coincide")
            g["pos"] = 0.5 * (ft[:3] + ft[3:])
            g["quat"] = _z_to_quat(d)
            g["size"] = np.array([g["size"][0], hl, 0.0])
        g["contype"] = int(dfl.get("geom", e, "contype", 1))
        g["conaffinity"] = int(dfl.get("geom", e, "conaffinity", 1))
        g["condim"] = int(dfl.get("geom", e, "condim", 3))
        g["friction"] = _floats(dfl.get("geom", e, "friction"), 3, DEFAULT_FRICTION)
        g["margin"] = float(dfl.get("geom", e, "margin", 0.0))
        g["gap"] = float(dfl.get("geom", e, "gap", 0.0))
        g["solref"] = _floats(dfl.get("geom", e, "solref"), 2, DEFAULT_SOLREF)
        g["solimp"] = _floats(dfl.get("geom", e, "solimp"), 5, DEFAULT_SOLIMP)
        g["density"] = float(dfl.get("geom", e, "density", DEFAULT_DENSITY))
        return g

    def parse_joint(e, bid):
        j = dict(body=bid, name=e.attrib.get("name", ""))
        t = dfl.get("joint", e, "type", "hinge")
        j["type"] = {"free": JNT_FREE, "ball": JNT_BALL, "slide": JNT_SLIDE, "hinge": JNT_HINGE}[t]
        j["pos"] = _floats(e.attrib.get("pos"), 3, [0, 0, 0])
        j["axis"] = _floats(dfl.get("joint", e, "axis"), 3, [0, 0, 1])
        j["limited"] = _bool(dfl.get("joint", e, "limited"), False)
        rng = _floats(dfl.get("joint", e, "range"), 2, [0, 0])
        if degree and j["type"] in (JNT_HINGE, JNT_BALL):
            rng = np.deg2rad(rng)
        j["range"] = rng
        j["armature"] = float(dfl.get("joint", e, "armature", 0.0))
        j["damping"] = float(dfl.get("joint", e, "damping", 0.0))
        j["stiffness"] = float(dfl.get("joint", e, "stiffness", 0.0))
        j["frictionloss"] = float(dfl.get("joint", e, "frictionloss", 0.0))
        j["springref"] = float(dfl.get("joint", e, "springref", 0.0))  # (MuJoCo's default is the joint's ref, which stays 0 here)
        if degree and j["type"] == JNT_HINGE:
            j["springref"] = float(np.deg2rad(j["springref"]))
        j["margin"] = float(dfl.get("joint", e, "margin", 0.0))
        if j["type"] == JNT_FREE:
            j["limited"] = False
        return j

    def walk(elem, parent_id):
        for e in elem:
            if e.tag == "geom":
                bodies[parent_id]["geoms"].append(parse_geom(e, parent_id))
            elif e.tag == "joint" or e.tag == "freejoint":
                if e.tag == "freejoint":
                    e.attrib["type"] = "free"
                bodies[parent_id]["joints"].append(parse_joint(e, parent_id))
            elif e.tag == "inertial":
                bodies[parent_id]["inertial"] = dict(pos=_floats(e.attrib.get("pos"), 3, [0, 0, 0]), quat=_floats(e.attrib.get("quat"), 4, [1, 0, 0, 0]),
                                                     mass=float(e.attrib["mass"]), diag=_floats(e.attrib.get("diaginertia"), 3, [0, 0, 0]))
            elif e.tag == "body":
                bid = len(bodies)
                b = dict(name=e.attrib.get("name", f"body{bid}"), parent=parent_id,
                         gpos=_floats(e.attrib.get("pos"), 3, [0, 0, 0]),
                         gquat=_floats(e.attrib.get("quat"), 4, [1, 0, 0, 0]), joints=[], geoms=[])
                b["gquat"] = b["gquat"] / np.linalg.norm(b["gquat"])
                bodies.append(b)
                walk(e, bid)

    walk(root.find("worldbody"), 0)

    # ---- global -> local frames ([MJ-ext] compiler coordinate="global") ----
    # after this every body has: pos/quat relative to parent, joints/geoms relative to body
    if global_coord:
        for b in bodies:
            b["wpos"], b["wquat"] = b["gpos"], b["gquat"]
    else:
        for i, b in enumerate(bodies):
            if i == 0:
                b["wpos"], b["wquat"] = b["gpos"], b["gquat"]
            else:
                p = bodies[b["parent"]]
                b["wpos"] = p["wpos"] + quat_to_mat(p["wquat"]) @ b["gpos"]
                b["wquat"] = quat_mul(p["wquat"], b["gquat"])
    for i, b in enumerate(bodies):
        if i == 0:
            b["pos"], b["quat"] = np.zeros(3), np.array([1.0, 0, 0, 0])
            continue
        p = bodies[b["parent"]]
        Rp = quat_to_mat(p["wquat"])
        b["pos"] = Rp.T @ (b["wpos"] - p["wpos"])
        b["quat"] = quat_mul(quat_conj(p["wquat"]), b["wquat"])
        Rb = quat_to_mat(b["wquat"])
        for j in b["joints"]:
            if global_coord:
                j["pos"] = Rb.T @ (j["pos"] - b["wpos"])
                j["axis"] = Rb.T @ j["axis"]
            n = np.linalg.norm(j["axis"])
            j["axis"] = j["axis"] / n if n > 0 else np.array([0, 0, 1.0])
            if j["type"] == JNT_FREE:
                j["pos"] = np.zeros(3)
    for i, b in enumerate(bodies):
        Rb = quat_to_mat(b["wquat"])
        for g in b["geoms"]:
            if global_coord and i > 0:
                g["pos"] = Rb.T @ (g["pos"] - b["wpos"])
                g["quat"] = quat_mul(quat_conj(b["wquat"]), g["quat"])

    # ---- sizes ----
    m.nbody = len(bodies)
    m.body_names = [b["name"] for b in bodies]
    joints = [j for b in bodies for j in b["joints"]]
    geoms = [g for b in bodies for g in b["geoms"]]
    m.njnt, m.ngeom = len(joints), len(geoms)
    m.joint_names = [j["name"] for j in joints]
    m.geom_names = [g["name"] for g in geoms]

    qn = {JNT_FREE: 7, JNT_BALL: 4, JNT_SLIDE: 1, JNT_HINGE: 1}
    vn = {JNT_FREE: 6, JNT_BALL: 3, JNT_SLIDE: 1, JNT_HINGE: 1}
    m.nq = sum(qn[j["type"]] for j in joints)
    m.nv = sum(vn[j["type"]] for j in joints)

    m.body_parentid = np.array([b["parent"] for b in bodies], dtype=np.int32)
    m.body_pos = np.array([b["pos"] for b in bodies])
    m.body_quat = np.array([b["quat"] for b in bodies])
    m.body_jntadr = np.zeros(m.nbody, dtype=np.int32)
    m.body_jntnum = np.zeros(m.nbody, dtype=np.int32)
    m.body_dofadr = np.zeros(m.nbody, dtype=np.int32)
    m.body_dofnum = np.zeros(m.nbody, dtype=np.int32)

    m.jnt_type = np.zeros(m.njnt, dtype=np.int32)
    m.jnt_bodyid = np.zeros(m.njnt, dtype=np.int32)
    m.jnt_qposadr = np.zeros(m.njnt, dtype=np.int32)
    m.jnt_dofadr = np.zeros(m.njnt, dtype=np.int32)
    m.jnt_pos = np.zeros((m.njnt, 3))
    m.jnt_axis = np.zeros((m.njnt, 3))
    m.jnt_limited = np.zeros(m.njnt, dtype=np.int32)
    m.jnt_range = np.zeros((m.njnt, 2))
    m.jnt_stiffness = np.zeros(m.njnt)
    m.jnt_margin = np.zeros(m.njnt)
    m.qpos0 = np.zeros(m.nq)
    m.dof_bodyid = np.zeros(m.nv, dtype=np.int32)
    m.dof_jntid = np.zeros(m.nv, dtype=np.int32)
    m.dof_parentid = np.full(m.nv, -1, dtype=np.int32)
    m.dof_armature = np.zeros(m.nv)
    m.dof_damping = np.zeros(m.nv)
    m.dof_frictionloss = np.zeros(m.nv)

    jid = qa = da = 0
    last_dof_of_body = np.full(m.nbody, -1, dtype=np.int32)
    for bid, b in enumerate(bodies):
        m.body_jntadr[bid] = jid if b["joints"] else -1
        m.body_jntnum[bid] = len(b["joints"])
        m.body_dofadr[bid] = da if b["joints"] else -1
        # first dof's parent = last dof of nearest ancestor that has dofs
        anc = b["parent"]
        prev = -1
        while bid > 0:
            if last_dof_of_body[anc] >= 0:
                prev = int(last_dof_of_body[anc])
                break
            if anc == 0:
                break
            anc = bodies[anc]["parent"]
        for j in b["joints"]:
            t = j["type"]
            m.jnt_type[jid] = t
            m.jnt_bodyid[jid] = bid
            m.jnt_qposadr[jid] = qa
            m.jnt_dofadr[jid] = da
            m.jnt_pos[jid] = j["pos"]
            m.jnt_axis[jid] = j["axis"]
            m.jnt_limited[jid] = int(j["limited"])
            m.jnt_range[jid] = j["range"]
            m.jnt_stiffness[jid] = j["stiffness"]
            m.jnt_margin[jid] = j["margin"]
            if t == JNT_FREE:
                m.qpos0[qa:qa + 3] = b["pos"]
                m.qpos0[qa + 3:qa + 7] = b["quat"]
            elif t == JNT_BALL:
                m.qpos0[qa] = 1.0
            for k in range(vn[t]):
                m.dof_bodyid[da] = bid
                m.dof_jntid[da] = jid
                m.dof_parentid[da] = prev
                m.dof_armature[da] = j["armature"]
                m.dof_damping[da] = j["damping"]
                m.dof_frictionloss[da] = j["frictionloss"]
                prev = da
                da += 1
            qa += qn[t]
            jid += 1
        m.body_dofnum[bid] = da - m.body_dofadr[bid] if b["joints"] else 0
        if b["joints"]:
            last_dof_of_body[bid] = da - 1
    m.qpos_spring = m.qpos0.copy()
    for jid, j in enumerate(joints):  # springref: the spring's rest position of a hinge / slide (ball and free joints rest at qpos0)
        if j["type"] in (JNT_SLIDE, JNT_HINGE):
            m.qpos_spring[m.jnt_qposadr[jid]] = j["springref"]
    # sparse-M row addresses: row i holds (i, parent(i), parent(parent(i)), ...) [MJ-ext qM layout]
    m.dof_madr = np.zeros(m.nv + 1, dtype=np.int32)
    for i in range(m.nv):
        depth, k = 0, i
        while k >= 0:
            depth += 1
            k = m.dof_parentid[k]
        m.dof_madr[i + 1] = m.dof_madr[i] + depth

    # ---- geoms + meshes; body inertial from geoms (inertiafromgeom) ----
    G = m.ngeom
    m.geom_type = np.array([g["type"] for g in geoms], dtype=np.int32)
    m.geom_bodyid = np.array([g["body"] for g in geoms], dtype=np.int32)
    m.geom_contype = np.array([g["contype"] for g in geoms], dtype=np.int32)
    m.geom_conaffinity = np.array([g["conaffinity"] for g in geoms], dtype=np.int32)
    m.geom_condim = np.array([g["condim"] for g in geoms], dtype=np.int32)
    m.geom_pos = np.array([g["pos"] for g in geoms]).reshape(G, 3)
    m.geom_quat = np.array([g["quat"] for g in geoms]).reshape(G, 4)
    m.geom_size = np.array([g["size"] for g in geoms]).reshape(G, 3)
    m.geom_friction = np.array([g["friction"] for g in geoms]).reshape(G, 3)
    m.geom_margin = np.array([g["margin"] for g in geoms])
    m.geom_gap = np.array([g["gap"] for g in geoms])
    m.geom_solref = np.array([g["solref"] for g in geoms]).reshape(G, 2)
    m.geom_solimp = np.array([g["solimp"] for g in geoms]).reshape(G, 5)
    m.geom_rbound = np.zeros(G)
    m.geom_center = np.zeros((G, 3))
    m.geom_vertadr = np.full(G, -1, dtype=np.int32)
    m.geom_vertnum = np.zeros(G, dtype=np.int32)

    m.body_mass = np.zeros(m.nbody)
    m.body_ipos = np.zeros((m.nbody, 3))
    m.body_iquat = np.tile(np.array([1.0, 0, 0, 0]), (m.nbody, 1))
    m.body_inertia = np.zeros((m.nbody, 3))
    acc = [dict(mass=0.0, mc=np.zeros(3), parts=[]) for _ in bodies]
    all_verts: List[np.ndarray] = []
    adj_adr: List[np.ndarray] = []
    adj_idx: List[np.ndarray] = []
    vbase = abase = 0
    for gi, g in enumerate(geoms):
        bid = g["body"]
        Rg = quat_to_mat(g["quat"])
        if g["type"] == GEOM_MESH:
            verts, faces = weld(mesh_tris[g["mesh"]])
            verts = verts @ Rg.T + g["pos"]  # -> body frame
            vol, com, I = polyhedron_mass_properties(verts, faces)
            mass = g["density"] * vol
            I = g["density"] * I
            adr, idx = hull_adjacency(len(verts), faces)
            m.geom_vertadr[gi] = vbase
            m.geom_vertnum[gi] = len(verts)
            all_verts.append(verts)
            adj_adr.append(adr[:-1] + abase)
            adj_idx.append(idx + vbase)
            vbase += len(verts)
            abase += len(idx)
            m.geom_center[gi] = com
            m.geom_rbound[gi] = np.linalg.norm(verts - com, axis=1).max()
            # geom frame == body frame for meshes in this build (vertices already moved)
            m.geom_pos[gi] = 0.0
            m.geom_quat[gi] = [1, 0, 0, 0]
        elif g["type"] == GEOM_BOX:
            sx, sy, sz = g["size"]
            mass = g["density"] * 8 * sx * sy * sz
            Il = mass / 3.0 * np.diag([sy * sy + sz * sz, sx * sx + sz * sz, sx * sx + sy * sy])
            I, com = Rg @ Il @ Rg.T, g["pos"]
            m.geom_center[gi] = com
            m.geom_rbound[gi] = np.linalg.norm(g["size"])
        elif g["type"] in (GEOM_SPHERE, GEOM_CAPSULE):
            # [MJ-ext] mjCGeom::SetInertia; for collisions the geom is a ROUNDED HULL: its core vertices (body frame) share the mesh tables
            r = g["size"][0]
            if g["type"] == GEOM_SPHERE:
                mass = g["density"] * 4.0 / 3.0 * np.pi * r ** 3
                Il = 0.4 * mass * r * r * np.eye(3)
                core = np.array([g["pos"]])
                nb = [[]]
            else:
                h = 2.0 * g["size"][1]
                mass = g["density"] * (np.pi * r * r * h + 4.0 / 3.0 * np.pi * r ** 3)
                ms = mass * 4 * r / (4 * r + 3 * h)  # the two half spheres
                mc = mass - ms
                ixx = mc * (3 * r * r + h * h) / 12 + 2 * ms * r * r / 5 + ms * h * (3 * r + 2 * h) / 8
                Il = np.diag([ixx, ixx, mc * r * r / 2 + 2 * ms * r * r / 5])
                axis = Rg[:, 2]
                core = np.array([g["pos"] + g["size"][1] * axis, g["pos"] - g["size"][1] * axis])  # [MJ-ext] mjc_PlaneCapsule's order: pos + segment first
                nb = [[1], [0]]
            I, com = Rg @ Il @ Rg.T, g["pos"]
            m.geom_vertadr[gi] = vbase
            m.geom_vertnum[gi] = len(core)
            all_verts.append(core)
            deg = np.array([len(l) for l in nb], dtype=np.int32)
            adj_adr.append((np.r_[0, np.cumsum(deg)][:-1] + abase).astype(np.int32))
            adj_idx.append(np.array([j for l in nb for j in l], dtype=np.int32) + vbase)
            vbase += len(core)
            abase += int(deg.sum())
            m.geom_center[gi] = com
            m.geom_rbound[gi] = r + (g["size"][1] if g["type"] == GEOM_CAPSULE else 0.0)
        else:  # plane: massless, unbounded
            continue
        if bid > 0:
            acc[bid]["mass"] += mass
            acc[bid]["mc"] += mass * com
            acc[bid]["parts"].append((mass, com, I))
    m.nmeshvert = vbase
    m.mesh_vert = np.concatenate(all_verts) if all_verts else np.zeros((0, 3))
    m.mesh_adjadr = np.concatenate(adj_adr + [np.array([abase], dtype=np.int32)]).astype(np.int32) if all_verts else np.zeros(1, dtype=np.int32)
    m.mesh_adj = np.concatenate(adj_idx).astype(np.int32) if all_verts else np.zeros(0, dtype=np.int32)
    m.nmeshadj = abase

    ifg = comp.get("inertiafromgeom", "auto")
    for bid in range(1, m.nbody):
        a = acc[bid]
        ine = bodies[bid].get("inertial")
        if ine is not None and ifg in ("false", "auto"):  # [MJ-ext] explicit <inertial> wins unless inertiafromgeom="true"
            if global_coord:
                Rb = quat_to_mat(bodies[bid]["wquat"])
                ine = dict(ine, pos=Rb.T @ (ine["pos"] - bodies[bid]["wpos"]), quat=quat_mul(quat_conj(bodies[bid]["wquat"]), ine["quat"]))
            m.body_mass[bid], m.body_ipos[bid] = ine["mass"], ine["pos"]
            m.body_iquat[bid], m.body_inertia[bid] = ine["quat"] / np.linalg.norm(ine["quat"]), ine["diag"]
            continue
        if a["mass"] <= 0:
            raise ValueError(f"body '{bodies[bid]['name']}' has no mass (inertiafromgeom needs a geom)")
        com = a["mc"] / a["mass"]
        I = np.zeros((3, 3))
        for mass, c, Ic in a["parts"]:
            d = c - com
            I += Ic + mass * (d @ d * np.eye(3) - np.outer(d, d))
        evals, evecs = np.linalg.eigh(I)
        order = np.argsort(-evals)  # [MJ-ext] principal moments in decreasing order
        evals, evecs = evals[order], evecs[:, order]
        if np.linalg.det(evecs) < 0:
            evecs[:, 2] = -evecs[:, 2]
        m.body_mass[bid] = a["mass"]
        m.body_ipos[bid] = com
        m.body_iquat[bid] = mat_to_quat(evecs)
        m.body_inertia[bid] = evals

    # ---- contact excludes ----
    ex = []
    c = root.find("contact")
    if c is not None:
        for e in c.findall("exclude"):
            ex.append([m.body_names.index(e.attrib["body1"]), m.body_names.index(e.attrib["body2"])])
    m.exclude_pair = np.array(ex, dtype=np.int32).reshape(-1, 2)
    m.nexclude = len(ex)

    # ---- actuators: motors on joints ----
    dofid, gear, names, crange = [], [], [], []
    act = root.find("actuator")
    if act is not None:
        for e in act:
            if e.tag not in ("motor", "general"):
                continue
            jn = e.attrib["joint"]
            j = m.joint_names.index(jn)
            if m.jnt_type[j] == JNT_FREE:
                raise ValueError("motors on free joints are not supported")
            dofid.append(m.jnt_dofadr[j])
            g = _floats(dfl.get("motor", e, "gear", "1"))
            gear.append(np.r_[g, np.zeros(3)][:3])  # [MJ-ext] gear[0] on scalar joints, gear[0..2] = torque vector on ball joints
            names.append(e.attrib.get("name", jn))
            crange.append(_floats(dfl.get("motor", e, "ctrlrange"), 2, [0, 0]))
    m.nu = len(dofid)
    m.actuator_dofid = np.array(dofid, dtype=np.int32)
    m.actuator_gear = np.array(gear, dtype=np.float64).reshape(-1, 3)
    m.actuator_names = names
    m.actuator_ctrlrange = np.array(crange, dtype=np.float64).reshape(-1, 2)

    set_const(m)
    return m


def compile_mjcf_file(path: str) -> Model:
    with open(path) as f:
        return compile_mjcf(f.read(), os.path.dirname(os.path.abspath(path)))


def scale_model(m: Model, s: float) -> Model:
    """Uniformly scaled copy of a model (all lengths x s at constant density): body offsets, inertial frames, hull
    vertices and bounding spheres scale with s, masses with s^3, inertias with s^5; the qpos0-derived constants are
    recomputed.  Same topology, so scaled models can share one batch (per-env shapes)."""
    o = m.copy()
    for name in ("body_pos", "body_ipos", "jnt_pos", "geom_pos", "geom_center", "mesh_vert"):
        setattr(o, name, getattr(m, name) * s)
    o.geom_rbound = m.geom_rbound * s
    o.geom_size = np.where(np.isin(m.geom_type, (GEOM_SPHERE, GEOM_CAPSULE, GEOM_BOX))[:, None], m.geom_size * s, m.geom_size)
    o.body_mass = m.body_mass * s ** 3
    o.body_inertia = m.body_inertia * s ** 5
    o.qpos0 = m.qpos0.copy()
    for j in range(m.njnt):
        if m.jnt_type[j] == JNT_FREE:
            a = m.jnt_qposadr[j]
            o.qpos0[a:a + 3] = m.qpos0[a:a + 3] * s
    o.qpos_spring = o.qpos0.copy()
    set_const(o)
    return o


def self_collision_variant(m: Model) -> Model:
    """The model with body-body collisions switched on, as the reference's GENERATED models have them (every body geom contype = 1,
    conaffinity = 1: uhc/smpllib/smpl_parser.py:327-328; Chest excluded against both shoulders: uhc/smpllib/smpl_robot.py:1177-1198).
    The shipped static asset is floor-only (contype 0); this is the same humanoid as the generator would emit it."""
    o = m.copy()
    o.geom_contype = m.geom_contype.copy()
    o.geom_contype[np.asarray(m.geom_bodyid) > 0] = 1
    ex = [list(p) for p in np.asarray(m.exclude_pair).reshape(-1, 2).tolist()]
    for a, b in (("Chest", "L_Shoulder"), ("Chest", "R_Shoulder")):
        if a in m.body_names and b in m.body_names:
            pair = [m.body_names.index(a), m.body_names.index(b)]
            if pair not in ex and pair[::-1] not in ex:
                ex.append(pair)
    o.exclude_pair = np.array(ex, dtype=np.int32).reshape(-1, 2)
    o.nexclude = len(ex)
    return o


def _rebuild_dof_tables(m: Model) -> None:
    """jnt_qposadr / jnt_dofadr / body_dofadr / body_dofnum / dof_* topology from (body tree, joints in body order, joint types)."""
    qn = {JNT_FREE: 7, JNT_BALL: 4, JNT_SLIDE: 1, JNT_HINGE: 1}
    vn = {JNT_FREE: 6, JNT_BALL: 3, JNT_SLIDE: 1, JNT_HINGE: 1}
    m.nq = int(sum(qn[int(t)] for t in m.jnt_type))
    m.nv = int(sum(vn[int(t)] for t in m.jnt_type))
    m.jnt_qposadr = np.zeros(m.njnt, dtype=np.int32)
    m.jnt_dofadr = np.zeros(m.njnt, dtype=np.int32)
    m.body_dofadr = np.full(m.nbody, -1, dtype=np.int32)
    m.body_dofnum = np.zeros(m.nbody, dtype=np.int32)
    m.dof_bodyid = np.zeros(m.nv, dtype=np.int32)
    m.dof_jntid = np.zeros(m.nv, dtype=np.int32)
    m.dof_parentid = np.full(m.nv, -1, dtype=np.int32)
    last = np.full(m.nbody, -1, dtype=np.int32)
    qa = da = 0
    for b in range(m.nbody):
        ja, jn = int(m.body_jntadr[b]), int(m.body_jntnum[b])
        prev, anc = -1, int(m.body_parentid[b])
        while b > 0:
            if last[anc] >= 0:
                prev = int(last[anc])
                break
            if anc == 0:
                break
            anc = int(m.body_parentid[anc])
        if jn:
            m.body_dofadr[b] = da
        for j in range(ja, ja + jn):
            t = int(m.jnt_type[j])
            m.jnt_qposadr[j], m.jnt_dofadr[j] = qa, da
            for _ in range(vn[t]):
                m.dof_bodyid[da], m.dof_jntid[da], m.dof_parentid[da] = b, j, prev
                prev = da
                da += 1
            qa += qn[t]
        if jn:
            m.body_dofnum[b] = da - m.body_dofadr[b]
            last[b] = da - 1
    m.dof_madr = np.zeros(m.nv + 1, dtype=np.int32)
    for i in range(m.nv):
        depth, k = 0, i
        while k >= 0:
            depth += 1
            k = int(m.dof_parentid[k])
        m.dof_madr[i + 1] = m.dof_madr[i] + depth


def ball_variant(m: Model, armature: float = 0.01, damping: float = 0.0) -> Model:
    """The humanoid with every (z, y, x) hinge triple replaced by ONE ball joint and three torque motors whose gear vectors are the
    old hinge axes -- the model `robot.ball: True` generates (uhc/khrylib/mocap/skeleton_mesh_v2.py:183-193 motors with gear = axis,
    :243-267 one `type="ball"` joint per bone; config/copycat_ball/copycat_ball_1.yml:99).  nq = 7 + 4 (nbody - 2), nv unchanged."""
    o = m.copy()
    jt, jb, jpos, names = [], [], [], []
    gear, act_j = [], []
    o.body_jntadr = np.full(m.nbody, -1, dtype=np.int32)
    o.body_jntnum = np.zeros(m.nbody, dtype=np.int32)
    for b in range(m.nbody):
        ja, jn = int(m.body_jntadr[b]), int(m.body_jntnum[b])
        if jn == 0:
            continue
        o.body_jntadr[b], o.body_jntnum[b] = len(jt), 1
        if jn == 1 and m.jnt_type[ja] == JNT_FREE:
            jt.append(JNT_FREE); jb.append(b); jpos.append(np.zeros(3)); names.append(m.joint_names[ja])
            continue
        assert jn == 3 and all(m.jnt_type[ja + k] == JNT_HINGE for k in range(3)), "ball_variant expects hinge triples"
        assert np.allclose(m.jnt_pos[ja], m.jnt_pos[ja + 1]) and np.allclose(m.jnt_pos[ja], m.jnt_pos[ja + 2])
        jt.append(JNT_BALL); jb.append(b); jpos.append(m.jnt_pos[ja].copy()); names.append(m.body_names[b])
        for k in range(3):
            act_j.append(len(jt) - 1)
            gear.append(m.jnt_axis[ja + k].copy())
    o.njnt = len(jt)
    o.joint_names = names
    o.jnt_type = np.array(jt, dtype=np.int32)
    o.jnt_bodyid = np.array(jb, dtype=np.int32)
    o.jnt_pos = np.array(jpos)
    o.jnt_axis = np.tile(np.array([0.0, 0, 1]), (o.njnt, 1))
    o.jnt_limited = np.zeros(o.njnt, dtype=np.int32)  # the generated ball joints carry no range
    o.jnt_range = np.zeros((o.njnt, 2))
    o.jnt_stiffness = np.zeros(o.njnt)
    o.jnt_margin = np.zeros(o.njnt)
    _rebuild_dof_tables(o)
    o.qpos0 = np.zeros(o.nq)
    for j in range(o.njnt):
        a = o.jnt_qposadr[j]
        if o.jnt_type[j] == JNT_FREE:
            o.qpos0[a:a + 7] = m.qpos0[m.jnt_qposadr[m.body_jntadr[o.jnt_bodyid[j]]]:][:7]
        else:
            o.qpos0[a] = 1.0
    o.qpos_spring = o.qpos0.copy()
    o.dof_armature = np.array([0.0 if o.jnt_type[o.dof_jntid[i]] == JNT_FREE else armature for i in range(o.nv)])
    o.dof_damping = np.array([0.0 if o.jnt_type[o.dof_jntid[i]] == JNT_FREE else damping for i in range(o.nv)])
    o.dof_frictionloss = np.zeros(o.nv)
    o.nu = len(gear)
    o.actuator_dofid = np.array([o.jnt_dofadr[j] for j in act_j], dtype=np.int32)
    o.actuator_gear = np.array(gear, dtype=np.float64).reshape(-1, 3)
    o.actuator_names = list(m.actuator_names)
    o.actuator_ctrlrange = np.zeros((o.nu, 2))
    set_const(o)
    return o


def hinge_to_ball_qpos(m_hinge: Model, m_ball: Model, qpos: np.ndarray) -> np.ndarray:
    """qpos of the hinge model -> the same pose of its ball variant (quaternion of R_z(a0) R_y(a1) R_x(a2) per body)."""
    out = m_ball.qpos0.copy()
    out[:7] = qpos[:7]
    for j in range(1, m_ball.njnt):
        if m_ball.jnt_type[j] != JNT_BALL:
            continue
        b = m_ball.jnt_bodyid[j]
        ja = m_hinge.body_jntadr[b]
        q = np.array([1.0, 0, 0, 0])
        for k in range(3):
            q = quat_mul(q, _axis_angle_quat(m_hinge.jnt_axis[ja + k], qpos[m_hinge.jnt_qposadr[ja + k]] - m_hinge.qpos0[m_hinge.jnt_qposadr[ja + k]]))
        a = m_ball.jnt_qposadr[j]
        out[a:a + 4] = q
    return out


def add_free_bodies(m: Model, hulls: List[np.ndarray], poses: np.ndarray, density: float = 1000.0, names: Optional[List[str]] = None,
                    contype: int = 1, conaffinity: int = 1, condim: int = 1, friction: Optional[float] = None) -> Model:
    """Append free-floating convex bodies (objects) to a model: one body, one free joint and one mesh geom each (the reference appends
    objects the same way: a body with a `free` joint and a mesh geom, contype = conaffinity = 1, uhc/smpllib/smpl_robot.py:1205-1224).
    hulls: list of (ntri, 3, 3) triangle soups in the object frame; poses: (K, 7) pos + quat of each object in qpos0."""
    o = m.copy()
    K = len(hulls)
    names = names or [f"obj{k}" for k in range(K)]
    g0 = m.ngeom - 1 if m.ngeom > 1 else 0  # geom whose contact parameters the objects copy (a body geom)
    for k, tris in enumerate(hulls):
        verts, faces = weld(np.asarray(tris, dtype=np.float64))
        vol, com, I = polyhedron_mass_properties(verts, faces)
        evals, evecs = np.linalg.eigh(density * I)
        order = np.argsort(-evals)
        evals, evecs = evals[order], evecs[:, order]
        if np.linalg.det(evecs) < 0:
            evecs[:, 2] = -evecs[:, 2]
        adr, idx = hull_adjacency(len(verts), faces)
        b, j, g = o.nbody, o.njnt, o.ngeom
        o.body_names = o.body_names + [names[k]]
        o.joint_names = o.joint_names + [names[k]]
        o.geom_names = o.geom_names + [names[k]]
        ap = lambda a, v: np.concatenate([a, np.asarray(v, dtype=a.dtype).reshape((1,) + a.shape[1:])])
        o.body_parentid = ap(o.body_parentid, 0); o.body_jntadr = ap(o.body_jntadr, j); o.body_jntnum = ap(o.body_jntnum, 1)
        o.body_dofadr = ap(o.body_dofadr, 0); o.body_dofnum = ap(o.body_dofnum, 6)
        o.body_pos = ap(o.body_pos, poses[k, :3]); o.body_quat = ap(o.body_quat, poses[k, 3:7] / np.linalg.norm(poses[k, 3:7]))
        o.body_ipos = ap(o.body_ipos, com); o.body_iquat = ap(o.body_iquat, mat_to_quat(evecs))
        o.body_mass = ap(o.body_mass, density * vol); o.body_inertia = ap(o.body_inertia, evals)
        o.body_invweight0 = ap(o.body_invweight0, [0.0, 0.0])
        o.jnt_type = ap(o.jnt_type, JNT_FREE); o.jnt_bodyid = ap(o.jnt_bodyid, b); o.jnt_qposadr = ap(o.jnt_qposadr, 0); o.jnt_dofadr = ap(o.jnt_dofadr, 0)
        o.jnt_pos = ap(o.jnt_pos, np.zeros(3)); o.jnt_axis = ap(o.jnt_axis, [0, 0, 1.0]); o.jnt_limited = ap(o.jnt_limited, 0)
        o.jnt_range = ap(o.jnt_range, [0.0, 0.0]); o.jnt_stiffness = ap(o.jnt_stiffness, 0.0); o.jnt_margin = ap(o.jnt_margin, 0.0)
        o.geom_type = ap(o.geom_type, GEOM_MESH); o.geom_bodyid = ap(o.geom_bodyid, b); o.geom_contype = ap(o.geom_contype, contype)
        o.geom_conaffinity = ap(o.geom_conaffinity, conaffinity); o.geom_condim = ap(o.geom_condim, condim)
        o.geom_pos = ap(o.geom_pos, np.zeros(3)); o.geom_quat = ap(o.geom_quat, [1.0, 0, 0, 0]); o.geom_size = ap(o.geom_size, np.zeros(3))
        for name in ("geom_friction", "geom_margin", "geom_gap", "geom_solref", "geom_solimp"):
            a = getattr(o, name)
            setattr(o, name, ap(a, a[g0]))
        if friction is not None:  # the reference writes friction="1 0.005 0.0001" on its object geoms (uhc/smpllib/smpl_robot.py:1216-1224)
            o.geom_friction[-1] = [float(friction), 0.005, 0.0001]
        o.geom_rbound = ap(o.geom_rbound, np.linalg.norm(verts - com, axis=1).max()); o.geom_center = ap(o.geom_center, com)
        o.geom_vertadr = ap(o.geom_vertadr, o.nmeshvert); o.geom_vertnum = ap(o.geom_vertnum, len(verts))
        o.mesh_adjadr = np.concatenate([o.mesh_adjadr[:-1], adr[:-1] + o.nmeshadj, [o.nmeshadj + len(idx)]]).astype(np.int32)
        o.mesh_adj = np.concatenate([o.mesh_adj, idx + o.nmeshvert]).astype(np.int32)
        o.mesh_vert = np.concatenate([o.mesh_vert, verts])
        o.nmeshvert += len(verts); o.nmeshadj += len(idx)
        o.nbody += 1; o.njnt += 1; o.ngeom += 1
    nq_old = m.nq
    _rebuild_dof_tables(o)
    q0 = np.zeros(o.nq)
    q0[:nq_old] = m.qpos0
    for k in range(K):
        a = o.jnt_qposadr[m.njnt + k]
        q0[a:a + 3] = poses[k, :3]
        q0[a + 3:a + 7] = poses[k, 3:7] / np.linalg.norm(poses[k, 3:7])
    o.qpos0, o.qpos_spring = q0, q0.copy()
    z6 = np.zeros(6 * K)
    o.dof_armature = np.concatenate([m.dof_armature, z6]); o.dof_damping = np.concatenate([m.dof_damping, z6])
    o.dof_frictionloss = np.concatenate([m.dof_frictionloss, z6])
    set_const(o)
    return o


def trailing_free_bodies(m: Model) -> int:
    """How many free bodies (objects: a body under the world with one free joint, no children) sit at the END of the model, behind the
    humanoid -- what `add_free_bodies` appends and the reference's `get_obj_qpos` reads as qpos[qpos_lim:] (uhc/envs/humanoid_im.py:1423-1428)."""
    k = 0
    for j in range(int(m.njnt) - 1, 0, -1):
        if int(m.jnt_type[j]) != JNT_FREE or int(m.body_parentid[int(m.jnt_bodyid[j])]) != 0 or int(m.jnt_bodyid[j]) != int(m.nbody) - 1 - k:
            break
        k += 1
    return k


def scale_model_per_body(m: Model, scales) -> Model:
    """Body-shape variation as SURVEY.md 8d config 4 prescribes: every body b gets its own length scale s_b (bone offsets of its
    children and its hull scale with s_b, mass with s_b^3, inertia with s_b^5 at constant density); the constants derived at qpos0
    are recomputed.  Same topology as `m`, so such models share one batch (one model blob per env)."""
    s = np.asarray(scales, dtype=np.float64)
    assert s.shape == (m.nbody,)
    o = m.copy()
    par = np.asarray(m.body_parentid)
    ps = np.where(par > 0, s[par], 1.0)  # a body's offset from its parent lives in the parent's frame: the parent's bone length
    o.body_pos = m.body_pos * ps[:, None]
    o.body_ipos = m.body_ipos * s[:, None]
    jb = np.asarray(m.jnt_bodyid)
    o.jnt_pos = m.jnt_pos * s[jb][:, None]
    gb = np.asarray(m.geom_bodyid)
    o.geom_pos = m.geom_pos * s[gb][:, None]
    o.geom_center = m.geom_center * s[gb][:, None]
    o.geom_rbound = m.geom_rbound * s[gb]
    o.geom_size = np.where(np.isin(m.geom_type, (GEOM_SPHERE, GEOM_CAPSULE, GEOM_BOX))[:, None], m.geom_size * s[gb][:, None], m.geom_size)
    mv = m.mesh_vert.copy()
    for g in range(m.ngeom):
        if m.geom_type[g] in HULL_TYPES:
            a, n = int(m.geom_vertadr[g]), int(m.geom_vertnum[g])
            mv[a:a + n] *= s[gb[g]]
    o.mesh_vert = mv
    o.body_mass = m.body_mass * s ** 3
    o.body_inertia = m.body_inertia * (s ** 5)[:, None]
    o.qpos0 = m.qpos0.copy()
    o.qpos_spring = o.qpos0.copy()
    set_const(o)
    return o


def export_mjcf(m: Model, density: Optional[float] = None) -> str:
    """The compiled model written back as MJCF in LOCAL coordinates (the reference's assets use `coordinate="global"`, which MuJoCo
    dropped after 2.x; this is the build's global -> local rewrite in file form).  Meshes are inlined as `vertex=` lists (body frame);
    MuJoCo takes their convex hull itself.  With `density` the bodies' inertial properties are left to the reader of the file
    (inertiafromgeom: what the reference's models do, density 1000); without, they are written out as `<inertial>` elements.
    Used to hand a model to a real MuJoCo where one is installed (tests/test_oracle_physics.py: the `import mujoco` comparison) and
    as the on-disk form of per-shape models."""
    f = lambda a: " ".join(repr(float(x)) for x in np.asarray(a).ravel())
    out = ['<mujoco model="uhc_amd_export">', '  <compiler angle="radian" inertiafromgeom="%s"/>' % ("true" if density is not None else "false"),
           f'  <option timestep="{m.timestep!r}" gravity="{f(m.gravity)}" iterations="{int(m.iterations)}" tolerance="{m.tolerance!r}"/>',
           '  <size njmax="2500" nconmax="500"/>', "  <asset>"]
    for g in range(m.ngeom):
        if m.geom_type[g] == GEOM_MESH:
            a, n = int(m.geom_vertadr[g]), int(m.geom_vertnum[g])
            out.append(f'    <mesh name="mesh{g}" vertex="{f(m.mesh_vert[a:a + n])}"/>')
    out += ["  </asset>", "  <worldbody>"]
    children: List[List[int]] = [[] for _ in range(m.nbody)]
    for b in range(1, m.nbody):
        children[int(m.body_parentid[b])].append(b)
    gtype = {GEOM_PLANE: "plane", GEOM_SPHERE: "sphere", GEOM_CAPSULE: "capsule", GEOM_BOX: "box", GEOM_MESH: "mesh"}

    def geoms_of(b, ind):
        for g in range(m.ngeom):
            if int(m.geom_bodyid[g]) != b:
                continue
            t = int(m.geom_type[g])
            s = (f'{ind}<geom name="{m.geom_names[g] or "geom%d" % g}" type="{gtype[t]}" contype="{int(m.geom_contype[g])}" '
                 f'conaffinity="{int(m.geom_conaffinity[g])}" condim="{int(m.geom_condim[g])}" friction="{f(m.geom_friction[g])}" '
                 f'margin="{float(m.geom_margin[g])!r}" gap="{float(m.geom_gap[g])!r}" solref="{f(m.geom_solref[g])}" solimp="{f(m.geom_solimp[g])}"')
            if t == GEOM_MESH:
                s += f' mesh="mesh{g}"'
            else:
                s += f' pos="{f(m.geom_pos[g])}" quat="{f(m.geom_quat[g])}" size="{f(m.geom_size[g])}"'
            if density is not None and b > 0:
                s += f' density="{float(density)!r}"'
            out.append(s + "/>")

    def emit(b, ind):
        out.append(f'{ind}<body name="{m.body_names[b]}" pos="{f(m.body_pos[b])}" quat="{f(m.body_quat[b])}">')
        if density is None:
            out.append(f'{ind}  <inertial pos="{f(m.body_ipos[b])}" quat="{f(m.body_iquat[b])}" mass="{float(m.body_mass[b])!r}" '
                       f'diaginertia="{f(m.body_inertia[b])}"/>')
        ja, jn = int(m.body_jntadr[b]), int(m.body_jntnum[b])
        for j in range(ja, ja + max(jn, 0)):
            t, d = int(m.jnt_type[j]), int(m.jnt_dofadr[j])
            name = m.joint_names[j] or f"joint{j}"
            if t == JNT_FREE:
                out.append(f'{ind}  <joint name="{name}" type="free" armature="{float(m.dof_armature[d])!r}" damping="{float(m.dof_damping[d])!r}"/>')
                continue
            kind = {JNT_BALL: "ball", JNT_SLIDE: "slide", JNT_HINGE: "hinge"}[t]
            out.append(f'{ind}  <joint name="{name}" type="{kind}" pos="{f(m.jnt_pos[j])}" axis="{f(m.jnt_axis[j])}" '
                       f'limited="{"true" if m.jnt_limited[j] else "false"}" range="{f(m.jnt_range[j])}" armature="{float(m.dof_armature[d])!r}" '
                       f'damping="{float(m.dof_damping[d])!r}" frictionloss="{float(m.dof_frictionloss[d])!r}" stiffness="{float(m.jnt_stiffness[j])!r}" '
                       f'margin="{float(m.jnt_margin[j])!r}"' + (f' springref="{float(m.qpos_spring[int(m.jnt_qposadr[j])])!r}"/>' if t != JNT_BALL else "/>"))
        geoms_of(b, ind + "  ")
        for c in children[b]:
            emit(c, ind + "  ")
        out.append(f"{ind}</body>")

    geoms_of(0, "    ")
    for c in children[0]:
        emit(c, "    ")
    out.append("  </worldbody>")
    if m.nexclude:
        out.append("  <contact>")
        for a, b in np.asarray(m.exclude_pair).reshape(-1, 2):
            out.append(f'    <exclude body1="{m.body_names[int(a)]}" body2="{m.body_names[int(b)]}"/>')
        out.append("  </contact>")
    if m.nu:
        out.append("  <actuator>")
        for a in range(m.nu):
            j = int(m.dof_jntid[int(m.actuator_dofid[a])])
            gear = np.atleast_1d(np.asarray(m.actuator_gear[a], dtype=np.float64))
            gs = f(gear) + " 0 0 0" if m.jnt_type[j] == JNT_BALL else repr(float(gear[0]))
            out.append(f'    <motor name="{m.actuator_names[a] or "motor%d" % a}" joint="{m.joint_names[j] or "joint%d" % j}" gear="{gs}"/>')
        out.append("  </actuator>")
    out.append("</mujoco>")
    return "\n".join(out) + "\n"


def common_mesh_layout(models: List[Model]) -> List[Model]:
    """Make models of one kinematic topology share ONE batch although their hulls differ (body shapes generated from different betas:
    uhc/envs/humanoid_im.py:154-190 rebuilds the model per clip; hulls are decimated to <= 50 vertices, smaller ones keep their own count).
    The batch wants the same vertex range per geom in every model: each geom is padded to the largest count it has in any of the models
    by repeating its FIRST vertex at the end.  A repeated vertex changes nothing: support queries break ties towards the lowest vertex
    id (plane-mesh arg-min and MPR's first arg-max, in the kernels and in the oracle alike), and the copies have no hull-graph
    neighbours.  Hull graphs stay per model (they travel in the model blobs)."""
    if len(models) < 2:
        return list(models)
    ng = models[0].ngeom
    assert all(m.ngeom == ng and np.array_equal(m.geom_type, models[0].geom_type) for m in models), "same geoms expected"
    vmax = np.max(np.stack([m.geom_vertnum for m in models]), axis=0)
    out = []
    for m in models:
        if np.array_equal(m.geom_vertnum, vmax):
            out.append(m)
            continue
        o = m.copy()
        verts, adr_new, remap = [], np.full(ng, -1, dtype=np.int32), np.full(m.nmeshvert, -1, dtype=np.int64)
        base = 0
        for g in range(ng):
            if m.geom_type[g] not in HULL_TYPES:
                continue
            a, n = int(m.geom_vertadr[g]), int(m.geom_vertnum[g])
            v = m.mesh_vert[a:a + n]
            verts.append(np.concatenate([v, np.repeat(v[:1], int(vmax[g]) - n, axis=0)]))
            adr_new[g] = base
            remap[a:a + n] = base + np.arange(n)
            base += int(vmax[g])
        o.mesh_vert = np.concatenate(verts) if verts else np.zeros((0, 3))
        o.nmeshvert = base
        o.geom_vertadr, o.geom_vertnum = adr_new, vmax.astype(np.int32)
        adjadr = np.zeros(base + 1, dtype=np.int32)
        deg = np.zeros(base, dtype=np.int32)
        old_deg = np.diff(m.mesh_adjadr)
        deg[remap[:m.nmeshvert]] = old_deg
        adjadr[1:] = np.cumsum(deg)
        adj = np.zeros(int(adjadr[-1]), dtype=np.int32)
        for v_old in range(m.nmeshvert):
            s, e = int(m.mesh_adjadr[v_old]), int(m.mesh_adjadr[v_old + 1])
            adj[adjadr[remap[v_old]]:adjadr[remap[v_old]] + (e - s)] = remap[m.mesh_adj[s:e]]
        o.mesh_adjadr, o.mesh_adj, o.nmeshadj = adjadr, adj, int(adjadr[-1])
        out.append(o)
    return out
