"""The SMPL body mesh: model files, the float64 host forward pass and the parser class of the reference (uhc/smpllib/smpl_parser.py:335-424
`SMPL_Parser.get_joints_verts`, `get_offsets`, `get_mesh_offsets`, which call smplx's lbs).

    load_smpl_model   the tables of one SMPL model file (.npz / .pkl of the SMPL authors, licensed and not shipped) as float64 arrays
    lbs_numpy         vertices and joints of posed bodies on the host: the arithmetic uhc_amd/csrc/uhc_smpl_mesh.hip computes on the device
    mesh_metrics_numpy  pen / skate / float / contact of a vertex sequence with smpl_eval's compute_* functions
    SMPL_Parser       get_joints_verts on device tensors through the kernel; get_offsets / get_mesh_offsets at the zero pose

SMPL-H and SMPL-X bodies are not served (their joint trees and feature widths differ): a file of theirs is refused by its posedirs shape."""
from __future__ import annotations

import os

import numpy as np

from .smpl_mujoco import SMPL_BONE_ORDER_NAMES
from .smpl_robot import SMPLBody

N_JOINT, N_BETA, N_FEAT = 24, 10, 207
MODEL_KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "kintree_table")
GENDERS = {"neutral": 0, "male": 1, "female": 2}


def gender_index(gender) -> int:
    g = gender.item() if isinstance(gender, np.ndarray) and gender.ndim == 0 else gender
    g = np.asarray(g).reshape(-1)[0] if isinstance(g, (np.ndarray, list, tuple)) else g
    g = g.decode("utf-8") if isinstance(g, bytes) else g
    if isinstance(g, str):
        if g not in GENDERS:
            raise Exception("Gender Not Supported!!")
        return GENDERS[g]
    if int(g) not in (0, 1, 2):
        raise Exception("Gender Not Supported!!")
    return int(g)


def _dense(a):
    return np.asarray(a.todense() if hasattr(a, "todense") else a)


def model_from_tables(z) -> dict:
    """A mapping with MODEL_KEYS -> the model as this module keeps it: float64, shapedirs (V, 3, 10), posedirs (V, 3, 207), J_regressor (24, V), weights
    (V, 24), parents int32 [24] with parents[0] = -1."""
    if "posedirs" not in z:
        raise ValueError("SMPL model without `posedirs`: the pose blend shapes are part of the mesh (a file reduced to v_template / shapedirs / J_regressor / "
                         "weights serves SMPLBody's zero pose only)")
    for k in MODEL_KEYS:
        if k not in z:
            raise ValueError(f"SMPL model without `{k}`")
    v = np.ascontiguousarray(_dense(z["v_template"]), dtype=np.float64)
    V = v.shape[0]
    sd = np.asarray(_dense(z["shapedirs"]), dtype=np.float64)
    if sd.shape[:2] != (V, 3) or sd.shape[2] < N_BETA:
        raise ValueError(f"SMPL model: shapedirs {sd.shape}, expected ({V}, 3, >= {N_BETA})")
    pd = np.asarray(_dense(z["posedirs"]), dtype=np.float64)
    if pd.shape == (N_FEAT, 3 * V):  # smplx's own layout: posedirs.reshape(V * 3, 207).T
        pd = pd.T.reshape(V, 3, N_FEAT)
    if pd.shape != (V, 3, N_FEAT):
        raise ValueError(f"SMPL model: posedirs {pd.shape}, expected ({V}, 3, {N_FEAT}) or ({N_FEAT}, {3 * V}) (SMPL-H / SMPL-X are not served)")
    jr = np.asarray(_dense(z["J_regressor"]), dtype=np.float64)
    w = np.asarray(_dense(z["weights"]), dtype=np.float64)
    if jr.shape != (N_JOINT, V) or w.shape != (V, N_JOINT):
        raise ValueError(f"SMPL model: J_regressor {jr.shape} / weights {w.shape}, expected ({N_JOINT}, {V}) / ({V}, {N_JOINT})")
    parents = np.asarray(_dense(z["kintree_table"])).reshape(2, -1)[0].astype(np.int64)
    parents = np.where((parents < 0) | (parents >= N_JOINT), -1, parents).astype(np.int32)  # (the files hold 2^32 - 1 for "no parent")
    if parents.shape != (N_JOINT,) or parents[0] != -1 or any(not 0 <= parents[j] < j for j in range(1, N_JOINT)):
        raise ValueError("SMPL model: kintree_table is no tree rooted at joint 0 with parent[j] < j")
    return dict(v_template=v, shapedirs=np.ascontiguousarray(sd[:, :, :N_BETA]), posedirs=np.ascontiguousarray(pd), J_regressor=np.ascontiguousarray(jr),
                weights=np.ascontiguousarray(w), parents=parents)


def load_smpl_model(path_or_dir, gender="neutral") -> dict:
    """The model file itself (.npz / .pkl), or the directory that holds SMPL_NEUTRAL / SMPL_MALE / SMPL_FEMALE (.npz before .pkl) with `gender` choosing."""
    path = str(path_or_dir)
    if os.path.isdir(path):
        stem = os.path.join(path, SMPLBody.FILES[gender_index(gender)])
        found = [stem + ext for ext in (".npz", ".pkl") if os.path.exists(stem + ext)]
        if not found:
            raise FileNotFoundError(f"SMPL model file {stem}.npz|.pkl not found: the SMPL body models are licensed and not shipped; place them under {path}")
        path = found[0]
    if path.endswith(".npz"):
        z = dict(np.load(path, allow_pickle=True))
        z = {k: (v.item() if isinstance(v, np.ndarray) and v.dtype == object and v.ndim == 0 else v) for k, v in z.items()}
    else:
        import pickle
        with open(path, "rb") as f:
            z = pickle.load(f, encoding="latin1")
    try:
        return model_from_tables(z)
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None


def rodrigues(r):
    """(..., 3) rotation vectors -> (..., 3, 3): smplx's batch_rodrigues -- the angle is |r + 1e-8|, the direction r / angle, no branch."""
    r = np.asarray(r, dtype=np.float64)
    a = np.sqrt(((r + 1e-8) ** 2).sum(axis=-1))
    d = r / a[..., None]
    K = np.zeros(r.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -d[..., 2], d[..., 1], d[..., 2], -d[..., 0], -d[..., 1], d[..., 0]
    return np.eye(3) + np.sin(a)[..., None, None] * K + (1.0 - np.cos(a))[..., None, None] * (K @ K)


def lbs_numpy(model, pose_aa, betas=None, trans=None):
    """pose_aa (T, 72), betas (10,) | (T, 10) | None, trans (T, 3) | None -> (vertices (T, V, 3), joints (T, 24, 3)), float64."""
    pose = np.asarray(pose_aa, dtype=np.float64).reshape(-1, N_JOINT, 3)
    T = pose.shape[0]
    b = np.zeros((1, N_BETA)) if betas is None else np.asarray(betas, dtype=np.float64).reshape(-1, np.shape(betas)[-1])[:, :N_BETA]
    tr = np.zeros((T, 3)) if trans is None else np.asarray(trans, dtype=np.float64).reshape(T, 3)
    v_shaped = model["v_template"][None] + np.einsum("vcb,tb->tvc", model["shapedirs"], b)  # (1 | T, V, 3)
    J = np.einsum("jv,tvc->tjc", model["J_regressor"], v_shaped)
    v_shaped, J = np.broadcast_to(v_shaped, (T,) + v_shaped.shape[1:]), np.broadcast_to(J, (T, N_JOINT, 3))
    R = rodrigues(pose)  # (T, 24, 3, 3)
    feature = (R[:, 1:] - np.eye(3)).reshape(T, N_FEAT)
    V = v_shaped.shape[1]
    v_posed = v_shaped + (feature @ model["posedirs"].reshape(V * 3, N_FEAT).T).reshape(T, V, 3)
    parents = model["parents"]
    GR, Gt = np.zeros((T, N_JOINT, 3, 3)), np.zeros((T, N_JOINT, 3))
    for j in range(N_JOINT):
        p = int(parents[j])
        if p < 0:
            GR[:, j], Gt[:, j] = R[:, j], J[:, j]
        else:
            GR[:, j] = GR[:, p] @ R[:, j]
            Gt[:, j] = np.einsum("tab,tb->ta", GR[:, p], J[:, j] - J[:, p]) + Gt[:, p]
    At = Gt - np.einsum("tjab,tjb->tja", GR, J)
    TR = np.einsum("vj,tjab->tvab", model["weights"], GR)
    Tt = np.einsum("vj,tja->tva", model["weights"], At)
    vert = np.einsum("tvab,tvb->tva", TR, v_posed) + Tt + tr[:, None]
    return vert, Gt + tr[:, None]


def mesh_metrics_numpy(vert, floor_z=0.0):
    """(T, V, 3) -> (rows (T, 4) in eval_ops.SURFACE_METRICS order -- the skate of the last row NaN --, means (4,): over T, T - 1, T, T rows)"""
    from . import smpl_eval as E
    info = {"floor_z": floor_z}
    T = vert.shape[0]
    rows = np.full((T, 4), np.nan)
    rows[:, 0], rows[:, 2], rows[:, 3] = E.compute_penetration(vert, info), E.compute_float(vert, info), E.compute_contact(vert, info)
    rows[:T - 1, 1] = E.compute_skate(vert, info)
    mean = lambda x: x.mean() if x.size else np.nan  # (np.mean of an empty array, without its warning)
    means = np.array([mean(rows[:, 0]), mean(rows[:T - 1, 1]), mean(rows[:, 2]), mean(rows[:, 3])])
    return rows, means


class SMPL_Parser:
    """The reference's SMPL_Parser, as far as this library is used through it: get_joints_verts runs uhc_smpl_mesh on the tensors' device (there is no host
    fall-back: host arrays go through lbs_numpy by name), get_offsets / get_mesh_offsets evaluate the zero pose on the host."""

    def __init__(self, model_path="data/smpl", gender="neutral", **_):
        self.model = load_smpl_model(model_path, gender)
        self.gender = gender
        self.parents = self.model["parents"]
        self.lbs_weights = self.model["weights"]
        self.joint_names = list(SMPL_BONE_ORDER_NAMES)
        # per joint, by name: identity axes, hinge order z, y, x, +-pi per hinge (the elbows four turns either way); every body collides with every other
        self.joint_axes, self.joint_dofs, self.joint_range = {}, {}, {}
        for name in self.joint_names:
            turns = 4.0 if name in ("L_Elbow", "R_Elbow") else 1.0
            self.joint_axes[name] = np.eye(3)
            self.joint_dofs[name] = list("zyx")
            self.joint_range[name] = np.tile([-turns * np.pi, turns * np.pi], (3, 1))
        self.contype = {1: self.joint_names}
        self.conaffinity = {1: self.joint_names}
        self._mesh = None

    def mesh(self):
        """The device handle (eval_ops.SmplMesh), made on first use on the current device."""
        if self._mesh is None:
            from ..eval_ops import SmplMesh
            self._mesh = SmplMesh([self.model])
        return self._mesh

    def get_joints_verts(self, pose, th_betas=None, th_trans=None):
        """pose (B, 72) or anything that reshapes to it, th_betas (1 | B, 10 | 16) or None, th_trans (B, 3) or None: device tensors ->
        (vertices (B, V, 3), joints (B, 24, 3)) float64 on the same device."""
        import torch
        from ..eval_ops import smpl_mesh
        if not (torch.is_tensor(pose) and pose.is_cuda):
            raise ValueError("SMPL_Parser.get_joints_verts takes device tensors (the mesh is computed by the HIP kernel); for host arrays call lbs_numpy")
        pose = pose.reshape(-1, 72).to(torch.float64).contiguous()
        B, dev = pose.shape[0], pose.device
        betas = torch.zeros(1, N_BETA, dtype=torch.float64, device=dev) if th_betas is None else th_betas.to(dev, torch.float64).reshape(-1, th_betas.shape[-1])
        betas = betas[:, :N_BETA].contiguous()  # (a width of 16 is cut to 10, as the reference does)
        trans = torch.zeros(B, 3, dtype=torch.float64, device=dev) if th_trans is None else th_trans.to(dev, torch.float64).reshape(B, 3).contiguous()
        if betas.shape[0] not in (1, B):
            raise ValueError(f"SMPL_Parser.get_joints_verts: {betas.shape[0]} betas for {B} poses")
        if betas.shape[0] == 1:  # one body: one sequence of B rows
            start, rows = torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), B, dtype=torch.int32, device=dev)
        else:                    # a body per pose: B sequences of one row
            start, rows = torch.arange(B, dtype=torch.int64, device=dev), torch.ones(B, dtype=torch.int32, device=dev)
        out = smpl_mesh(self.mesh(), pose, trans, start, rows, betas, want=("vertices", "joints"), row_cap=max(B, 1) if betas.shape[0] == 1 else 1)
        return out["vertices"], out["joints"]

    def _zero_pose(self, betas):
        b = np.zeros(N_BETA) if betas is None else np.asarray(betas.detach().cpu().numpy() if hasattr(betas, "detach") else betas, dtype=np.float64).reshape(-1)[:N_BETA]
        vert, jts = lbs_numpy(self.model, np.zeros((1, 72)), b)
        return vert[0], jts[0]

    def _tree(self, jts, root_offset):
        """bone vectors and parent names of the 24 joints by name, from the joint positions; the root gets `root_offset` and `root_parent`"""
        offsets, parents = {}, {}
        for j, name in enumerate(self.joint_names):
            p = int(self.parents[j])
            offsets[name] = root_offset.copy() if j == 0 else jts[j] - jts[p]
            parents[name] = self.joint_names[p] if p >= 0 else None
        return offsets, parents

    def get_offsets(self, betas=None):
        """-> (joint offsets by name, parent names, channels, joint ranges) at the zero pose; the root's offset is zero.  The reference indexes its name list
        with the root's parent, -1, so the root's "parent" reads as the last joint's name (smpl_parser.py:362-384); kept."""
        _, jts = self._zero_pose(betas)
        offsets, parents = self._tree(jts, np.zeros(3))
        parents[self.joint_names[0]] = self.joint_names[-1]
        return offsets, parents, list("zyx"), self.joint_range

    def get_mesh_offsets(self, betas=None, flatfoot=False):
        """-> (verts, joint_pos, skin_weights, joint_names, joint_offsets, joint_parents, joint_axes, joint_dofs, joint_range, contype, conaffinity) at the
        zero pose; the root's offset is its position, its parent None; flatfoot puts the vertices within 1 cm of the lowest y onto their mean y
        (smpl_parser.py:386-424)."""
        verts, jts = self._zero_pose(betas)
        if flatfoot:
            sole = np.flatnonzero(verts[:, 1] < verts[:, 1].min() + 0.01)
            verts[sole, 1] = verts[sole, 1].mean()
        offsets, parents = self._tree(jts, jts[0])
        return (verts, jts, self.lbs_weights, self.joint_names, offsets, parents, self.joint_axes, self.joint_dofs, self.joint_range, self.contype, self.conaffinity)


class MeshBodyProvider:
    """(betas, gender) -> (vertices, joints, skin weights) at the zero pose, like SMPLBody, from full model files; keeps the models for the mesh kernel."""

    def __init__(self, data_dir="data/smpl"):
        self.data_dir = data_dir
        self._models = {}

    def model(self, gender) -> dict:
        g = gender_index(gender)
        if g not in self._models:
            self._models[g] = load_smpl_model(self.data_dir, g)
        return self._models[g]

    def __call__(self, betas, gender=0):
        m = self.model(gender)
        vert, jts = lbs_numpy(m, np.zeros((1, 72)), np.asarray(betas, dtype=np.float64).reshape(-1)[:N_BETA])
        return vert[0], jts[0], m["weights"]
