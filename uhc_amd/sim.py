"""Batched simulation handle over the C-ABI (include/uhc_amd.h).  torch is used only for device
memory and streams; every computation happens inside libuhc_amd.so."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np
import torch

from ._capi import UhcCtrlDesc, UhcEnvDesc, model_desc
from ._capi import (DEBUG_ENV_ORDER, DEBUG_EXP_FILL_48, DEBUG_EXP_FILL_56, DEBUG_EXP_FIXED_CAP2, DEBUG_EXP_MASK, DEBUG_EXP_NO_RANK_FILL, DEBUG_EXP_STICKY_TIER4,  # noqa: F401
                    DEBUG_LOG, DEBUG_NO_BOX_CULL, DEBUG_NO_GATE, DEBUG_NO_MERGE, DEBUG_NO_VSTAGE, DEBUG_RESTART_HANDON, DEBUG_TRACE, PROF_WORDS, TRACE_CHUNK_WAIT,
                    TRACE_CONSUMER, TRACE_CONSUMER_WORDS, TRACE_GATE, TRACE_HANDON_SUBSTEP, TRACE_HANDON_SUBSTEP3, TRACE_LET_GO, TRACE_LET_GO4, TRACE_TAKEN, TRACE_TAKEN4)
from ._capi import (REDO_DROPPED, REDO_GENERAL, REDO_LARGE, REDO_PRIMAL, REDO_PRIMAL_CAP, REDO_SWEPT, REDO_SWEPT_SUBSTEP0, REDO_SWEPT_SUBSTEPS,  # noqa: F401 (re-exported next to F_*)
                    REDO_WHY_FRICTION, REDO_WHY_NOCONV, REDO_WHY_PIVOT, REDO_WINDOWED, WHY_CANDIDATES, WHY_CONTACTS, WHY_DENSE_SLOTS, WHY_FAST_SHIFT, WHY_FIELD,
                    WHY_GENERAL_SHIFT, WHY_LARGE_SHIFT, WHY_ROW_STORAGE, WHY_ROWS, WHY_SOLVER, WHY_SUBSTEP_SHIFT)
from ._lib import check, lib

F_QPOS, F_QVEL, F_XPOS, F_XQUAT, F_XIPOS, F_QM, F_QFRC_BIAS, F_QACC, F_CTRL = range(9)
F_NCON, F_NEFC, F_FAIL, F_SOLVER_ITER, F_QFRC_APPLIED, F_EFC_OVERFLOW, F_STAGE_PROF, F_REDO, F_TIER, F_HANDON_WHY = range(9, 19)
F_QACC_WARMSTART, F_COST = 19, 20
_INT_FIELDS = {F_NCON, F_NEFC, F_FAIL, F_SOLVER_ITER, F_EFC_OVERFLOW, F_REDO, F_TIER, F_HANDON_WHY, F_COST}


class _DevView:
    """__cuda_array_interface__ view of library-owned device memory (no copy, no ownership)."""

    def __init__(self, ptr: int, shape, typestr: str, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 2}
        self._owner = owner


_DEFERRED = []  # handles whose owner was finalised while a stream was capturing: freed by the next close() / SimBatch creation outside a capture


def _capturing() -> bool:
    try:
        return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
    except Exception:
        return False


def _drain_deferred() -> None:
    if not _DEFERRED or _capturing():
        return
    pending, _DEFERRED[:] = list(_DEFERRED), []
    for L, kind, h, models in sorted(pending, key=lambda x: x[1] != "env"):  # env layers before the batches they sit on
        if kind == "env":
            L.uhc_env_free(h)
        else:
            L.uhc_batch_free(h)
            for mh in models:
                L.uhc_model_free(mh)


class SimBatch:
    def __init__(self, models, ctrl: UhcCtrlDesc, n_env: int, env_model: Optional[Sequence[int]] = None, device: int = 0):
        if not isinstance(models, (list, tuple)):
            models = [models]
        if not torch.cuda.is_available():
            raise RuntimeError("uhc_amd.SimBatch needs an MI355X (torch.cuda unavailable); there is no CPU fallback")
        self.L = lib()
        self.models = list(models)
        self.model = self.models[0]
        self.n_env = int(n_env)
        self.device = torch.device("cuda", device)
        self.ctrl = ctrl
        self._descs = [model_desc(m) for m in self.models]
        _drain_deferred()
        self._mh = []
        for d in self._descs:
            h = C.c_void_p()
            check(self.L.uhc_model_create(C.byref(d), C.byref(h)))
            self._mh.append(h)
        arr = (C.c_void_p * len(self._mh))(*[h.value for h in self._mh])
        em = None
        if env_model is not None:
            em_np = np.ascontiguousarray(env_model, dtype=np.int32)
            assert em_np.shape == (n_env,)
            em = em_np.ctypes.data_as(C.POINTER(C.c_int32))
        self._b = C.c_void_p()
        check(self.L.uhc_batch_create(arr, len(self._mh), em, self.n_env, device, C.byref(ctrl), C.byref(self._b)))
        self.nM = self.L.uhc_model_nM(self._mh[0])
        self._fields = {}
        self.use_current_stream()

    def close(self):
        if getattr(self, "_b", None) is not None and self._b:
            if _capturing():  # (a finaliser that fires inside a stream capture: hipFree is not allowed there -- the handles wait for the next close / creation)
                _DEFERRED.append((self.L, "batch", self._b, list(self._mh)))
                self._b, self._mh = None, []
                return
            _drain_deferred()
            self.L.uhc_batch_free(self._b)
            self._b = None
            for h in self._mh:
                self.L.uhc_model_free(h)
            self._mh = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- zero-copy torch views of the library-owned state
    def field(self, f: int) -> torch.Tensor:
        if f in self._fields:
            return self._fields[f]
        p, n = C.c_void_p(), C.c_int64()
        check(self.L.uhc_batch_field(self._b, f, C.byref(p), C.byref(n)))
        per = n.value // self.n_env
        if f == F_STAGE_PROF:
            t = torch.as_tensor(_DevView(p.value, (self.n_env, PROF_WORDS), "<i8", self), device=self.device)
        elif f in _INT_FIELDS:
            t = torch.as_tensor(_DevView(p.value, (self.n_env,), "<i4", self), device=self.device)
        else:
            t = torch.as_tensor(_DevView(p.value, (self.n_env, per), "<f8", self), device=self.device)
        self._fields[f] = t
        return t

    def use_current_stream(self):
        check(self.L.uhc_batch_set_stream(self._b, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def sync(self):
        check(self.L.uhc_batch_sync(self._b))

    def set_overflow_mode(self, truncate: bool):
        """False (default): envs beyond the fast kernel's 16 contacts / 64 rows are redone exactly by the general kernel;
        True: they keep what fits (reported in F_EFC_OVERFLOW) and no second pass is needed."""
        check(self.L.uhc_batch_set_overflow_mode(self._b, int(bool(truncate))))

    def set_kernel_path(self, mode):
        """0 / False: tier chain (fast kernel, then the general tier on the envs beyond its capacity, then the large tier); 1 / True: general
        tier first (scenes where most envs exceed the fast kernel's 64 rows); 2: sticky tiers -- every env starts in the tier that computed
        its last step, the slower tiers run beside the fast one on a side stream (include/uhc_amd.h)."""
        check(self.L.uhc_batch_set_kernel_path(self._b, int(mode)))

    def set_solver(self, solver: int, iterations: int = 0):
        """Contact solver of the following launches: 0 = PGS sweeps (cap `iterations`), 1 = exact active-set solve."""
        check(self.L.uhc_batch_set_solver(self._b, int(solver), int(iterations)))

    def set_rfc_scale(self, s: float):
        check(self.L.uhc_batch_set_rfc_scale(self._b, float(s)))

    def set_state(self, qpos: torch.Tensor, qvel: torch.Tensor, env_ids: Optional[torch.Tensor] = None):
        qpos = qpos.to(self.device, torch.float64).contiguous()
        qvel = qvel.to(self.device, torch.float64).contiguous()
        n = qpos.shape[0]
        # the library reads n x nq and n x nv doubles: a pose of another model's width (a hinge pose handed to the ball-joint model) is a read
        # past the tensor and a humanoid put together from whatever lies there
        if qpos.ndim != 2 or qvel.ndim != 2 or qpos.shape[1] != self.model.nq or qvel.shape != (n, self.model.nv):
            raise ValueError(f"set_state: qpos {tuple(qpos.shape)} / qvel {tuple(qvel.shape)} for a model with nq {self.model.nq}, nv {self.model.nv}")
        ids = None
        if env_ids is not None:
            env_ids = env_ids.to(self.device, torch.int32).contiguous()
            assert env_ids.shape[0] == n
            ids = C.c_void_p(env_ids.data_ptr())
        check(self.L.uhc_batch_set_state(self._b, ids, n, C.c_void_p(qpos.data_ptr()), C.c_void_p(qvel.data_ptr())))
        self._keep = (qpos, qvel, env_ids)

    def simulate(self, action: torch.Tensor, target_base: torch.Tensor, active: Optional[torch.Tensor] = None):
        assert action.dtype == torch.float64 and action.is_contiguous() and action.shape == (self.n_env, self.ctrl.action_dim)
        if self.model.nu == 0:  # unactuated model: the library still wants non-null buffers
            target_base = action
        assert target_base.dtype == torch.float64 and target_base.is_contiguous() and (self.model.nu == 0 or target_base.shape == (self.n_env, self.model.nu))
        a = None
        if active is not None:
            assert active.dtype == torch.int32 and active.is_contiguous()
            a = C.c_void_p(active.data_ptr())
        check(self.L.uhc_batch_simulate(self._b, C.c_void_p(action.data_ptr()), C.c_void_p(target_base.data_ptr()), a))

    def forward(self):
        check(self.L.uhc_batch_forward(self._b))

    def set_timing(self, enable: bool):
        check(self.L.uhc_batch_set_timing(self._b, int(enable)))

    def kernel_time(self):
        """(total ms, launches) of the fused step kernel since the last call (HIP events on the batch's stream)."""
        ms, n = C.c_double(), C.c_int32()
        check(self.L.uhc_batch_kernel_time(self._b, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def give_ups(self) -> int:
        """Workgroups that gave up waiting (queue consumers, chunk waiters) since the batch was created; 0 in a healthy run."""
        n = C.c_int32()
        check(self.L.uhc_batch_give_ups(self._b, C.byref(n), None))
        return n.value

    def slow_leaves(self) -> int:
        """Queue consumers that left after 50 ms behind producers that were running but had not all finished (a very slow env-step in the tier below)."""
        n, m = C.c_int32(), C.c_int32()
        check(self.L.uhc_batch_give_ups(self._b, C.byref(n), C.byref(m)))
        return m.value


E_OBS, E_REWARD, E_REWARD_PARTS, E_DONE, E_FAIL, E_END, E_PERCENT, E_CUR_T, E_BODY_DIFF, E_TARGET_BASE, E_CONSUMED, E_EPISODE, E_SNAPSHOT, E_MODEL = range(14)
_E_ROWS = {E_EPISODE: 2, E_SNAPSHOT: 5}  # fields laid out [rows][n_env]
_E_INT = {E_DONE, E_FAIL, E_END, E_CUR_T, E_CONSUMED, E_MODEL}
FRAME_STRIDE = 584
FR = dict(qpos=(0, 76), qvel=(76, 75), wbpos=(151, 72), wbquat=(223, 96), bquat=(319, 96), bangvel=(415, 72), ee_wpos=(487, 15), com=(502, 3), body_com=(512, 72))


def pack_expert_frames(feat) -> np.ndarray:
    """Expert feature dict (Humanoid.qpos_fk output) -> (T, FRAME_STRIDE) frame records of the clip bank."""
    T = int(feat["len"])
    out = np.zeros((T, FRAME_STRIDE))
    for k, (o, n) in FR.items():
        out[:, o:o + n] = np.asarray(feat[k]).reshape(T, n)
    return out


def expert_pose_of_frames(frames, ball: bool):
    """(qpos, qvel) of the model's own coordinates from frame records of the clip bank (numpy or torch, rows = frames): hinge angles as
    they are; ball joints -- root pose + the joints' quaternions (the record's body quaternions behind the root's), as the device-side
    reset builds it (uhc_env.hip: expert_qpos)."""
    import torch as _t
    cat = _t.cat if isinstance(frames, _t.Tensor) else np.concatenate
    q0, qn = FR["qpos"]
    b0, bn = FR["bquat"]
    v0, vn = FR["qvel"]
    qpos = cat([frames[:, q0:q0 + 7], frames[:, b0 + 4:b0 + bn]], 1) if ball else frames[:, q0:q0 + qn]
    return qpos, frames[:, v0:v0 + vn]


def expert_frames_device(qpos, clip_start, humanoids, clip_model=None, root_quat_record=None, dt: float = 1 / 30, device=None) -> torch.Tensor:
    """The clip bank's frame records computed on the device (uhc_expert_frames): what `pack_expert_frames(Humanoid.qpos_fk(clip))`, clip by
    clip, gives on the host, from ONE upload of the thin qpos rows and ONE launch on torch's current stream.
      qpos (n_frames, 76): the clips' hinge qpos one after another (numpy or torch, host or device); clip_start: first row of every clip;
      humanoids: one `Humanoid` (or a list of them, same tree) per body shape -- their offset tables are uploaded once --, clip_model: which of
      them each clip is computed with (None: the first for every clip); root_quat_record (n_frames, 4): written into the records' qpos[3:7]
      instead of qpos' own quaternion, which kinematics and velocities keep reading.
    Returns the (n_frames, FRAME_STRIDE) float64 device tensor `EnvBatch.set_bank` takes without a copy.  A clip of one frame gets zero qvel / bangvel."""
    if not torch.cuda.is_available():
        raise RuntimeError("uhc_amd.sim.expert_frames_device needs an MI355X (torch.cuda unavailable); there is no CPU fallback")
    hs = list(humanoids) if isinstance(humanoids, (list, tuple)) else [humanoids]
    if device is None:
        device = qpos.device if isinstance(qpos, torch.Tensor) and qpos.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    parents = np.ascontiguousarray(hs[0]._parents, dtype=np.int32)
    ee = np.ascontiguousarray(hs[0]._ee_idx, dtype=np.int32)
    for h in hs[1:]:
        if not np.array_equal(np.asarray(h._parents), parents) or list(h._ee_idx) != list(ee):
            raise ValueError("expert_frames_device: every body shape must share the first one's tree")
    if ee.shape != (5,):
        raise ValueError("expert_frames_device: five end effectors (SMPL_EE_NAMES) are what the frame record holds")
    cs = np.asarray(clip_start.cpu() if isinstance(clip_start, torch.Tensor) else clip_start, dtype=np.int64).reshape(-1)
    qpos = torch.as_tensor(qpos)
    n_frames = int(qpos.shape[0])
    if qpos.ndim != 2 or qpos.shape[1] != 76:
        raise ValueError(f"expert_frames_device: qpos must be (n_frames, 76), got {tuple(qpos.shape)}")
    if cs.size == 0 or cs[0] != 0 or np.any(np.diff(cs) <= 0) or (n_frames and cs[-1] >= n_frames):
        raise ValueError("expert_frames_device: clip_start must ascend strictly from 0 and stay below n_frames")
    cm = None
    if clip_model is not None:
        cm = np.asarray(clip_model.cpu() if isinstance(clip_model, torch.Tensor) else clip_model, dtype=np.int64).reshape(-1)
        if cm.shape != cs.shape or cm.min() < 0 or cm.max() >= len(hs):
            raise ValueError(f"expert_frames_device: clip_model must name one of the {len(hs)} body shapes for each of the {cs.size} clips")
    if n_frames == 0:
        return torch.empty((0, FRAME_STRIDE), dtype=torch.float64, device=device)
    with torch.cuda.device(device):  # (the temporaries below are freed in stream order: the launch is on torch's current stream)
        off = torch.stack([h._offsets for h in hs]).to(device, torch.float64).contiguous()
        ioff = torch.stack([h._i_offsets for h in hs]).to(device, torch.float64).contiguous()
        q = qpos.to(device, torch.float64).contiguous()
        d_cs = torch.from_numpy(cs.astype(np.int32)).to(device)
        d_cm = None if cm is None else torch.from_numpy(cm.astype(np.int32)).to(device)
        rq = None
        if root_quat_record is not None:
            rq = torch.as_tensor(root_quat_record).to(device, torch.float64).contiguous()
            if rq.shape != (n_frames, 4):
                raise ValueError(f"expert_frames_device: root_quat_record must be ({n_frames}, 4), got {tuple(rq.shape)}")
        out = torch.empty((n_frames, FRAME_STRIDE), dtype=torch.float64, device=device)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        check(lib().uhc_expert_frames(C.c_void_p(torch.cuda.current_stream(device).cuda_stream), int(off.shape[1]),
                                      parents.ctypes.data_as(C.POINTER(C.c_int32)), ee.ctypes.data_as(C.POINTER(C.c_int32)), ptr(off), ptr(ioff), len(hs),
                                      ptr(q), n_frames, ptr(d_cs), ptr(d_cm), int(cs.size), ptr(rq), float(dt), ptr(out)))
    return out


def smpl_qpos_device(pose_aa, trans, clip_start, models, clip_model=None, count_offset: bool = True, want=("qpos",), device=None):
    """AMASS axis-angle poses -> qpos rows on the device (uhc_smpl_qpos): what `smpl_to_qpose(clip, model)`, clip by clip, gives on the host, from
    ONE upload of the raw arrays and ONE launch on torch's current stream.
      pose_aa (n_frames, 72) and trans (n_frames, 3) or None: the clips one after another (numpy or torch, host or device); clip_start: first row of
      every clip; models: one compiled `Model` (or a list of them, same body order) per body shape -- their root offsets (body_pos[1]) are uploaded
      once and added to the root position when count_offset --, clip_model: which of them each clip is converted for (None: the first for every
      clip); want: ("qpos",), ("qpos_quat",) or both -- the hinge humanoid's 76-wide rows, the ball-joint humanoid's 99-wide rows.
    Returns the float64 device tensors in the order of `want`; they go into `expert_frames_device` as they are."""
    if not torch.cuda.is_available():
        raise RuntimeError("uhc_amd.sim.smpl_qpos_device needs an MI355X (torch.cuda unavailable); there is no CPU fallback")
    ms = list(models) if isinstance(models, (list, tuple)) else [models]
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or len(set(want)) != len(want) or any(w not in ("qpos", "qpos_quat") for w in want):
        raise ValueError(f"smpl_qpos_device: want names 'qpos' and / or 'qpos_quat', got {want!r}")
    if device is None:
        device = pose_aa.device if isinstance(pose_aa, torch.Tensor) and pose_aa.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    s2m = _smpl_table(ms, "smpl_qpos_device")
    pose = torch.as_tensor(pose_aa)
    n_frames = int(pose.shape[0])
    if pose.ndim < 2 or pose.numel() != n_frames * 72:
        raise ValueError(f"smpl_qpos_device: pose_aa must be (n_frames, 72) or (n_frames, 24, 3), got {tuple(pose.shape)}")
    pose = pose.reshape(n_frames, 72)
    if trans is not None:
        trans = torch.as_tensor(trans)
        if tuple(trans.shape) != (n_frames, 3):
            raise ValueError(f"smpl_qpos_device: trans must be ({n_frames}, 3), got {tuple(trans.shape)}")
    cs, cm = _clip_tables("smpl_qpos_device", clip_start, clip_model, n_frames, len(ms))
    widths = dict(qpos=76, qpos_quat=99)
    with torch.cuda.device(device):  # (the temporaries below are freed in stream order: the launch is on torch's current stream)
        out = {w: torch.empty((n_frames, widths[w]), dtype=torch.float64, device=device) for w in want}
        if n_frames:
            off = torch.from_numpy(np.stack([np.asarray(m.body_pos, dtype=np.float64)[1] for m in ms])).to(device).contiguous() if count_offset else None
            p = pose.to(device, torch.float64).contiguous()
            t = None if trans is None else trans.to(device, torch.float64).contiguous()
            d_cs = torch.from_numpy(cs.astype(np.int32)).to(device)
            d_cm = None if cm is None else torch.from_numpy(cm.astype(np.int32)).to(device)
            ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
            check(lib().uhc_smpl_qpos(C.c_void_p(torch.cuda.current_stream(device).cuda_stream), 24, s2m.ctypes.data_as(C.POINTER(C.c_int32)), ptr(off), len(ms),
                                      ptr(p), ptr(t), n_frames, ptr(d_cs), ptr(d_cm), int(cs.size), ptr(out.get("qpos")), ptr(out.get("qpos_quat"))))
    return tuple(out[w] for w in want)


def _clip_tables(who, clip_start, clip_model, n_frames, n_models):
    """-> (clip_start, clip_model or None) as int64 host arrays, checked: the starts ascend strictly from 0 below n_frames, the models are in range"""
    cs = np.asarray(clip_start.cpu() if isinstance(clip_start, torch.Tensor) else clip_start, dtype=np.int64).reshape(-1)
    if cs.size == 0 or cs[0] != 0 or np.any(np.diff(cs) <= 0) or (n_frames and cs[-1] >= n_frames):
        raise ValueError(f"{who}: clip_start must ascend strictly from 0 and stay below n_frames")
    cm = None
    if clip_model is not None:
        cm = np.asarray(clip_model.cpu() if isinstance(clip_model, torch.Tensor) else clip_model, dtype=np.int64).reshape(-1)
        if cm.shape != cs.shape or cm.min() < 0 or cm.max() >= n_models:
            raise ValueError(f"{who}: clip_model must name one of the {n_models} body shapes for each of the {cs.size} clips")
    return cs, cm


def _smpl_table(ms, who):
    from .smpllib.smpl_mujoco import smpl_to_model_table
    tables = [smpl_to_model_table(m) for m in ms]
    if any(t != tables[0] for t in tables[1:]):
        raise ValueError(f"{who}: every body shape must share the first one's body order")
    s2m = np.ascontiguousarray(tables[0], dtype=np.int32)
    if s2m.shape != (24,):
        raise ValueError(f"{who}: the model carries {s2m.size} of the 24 SMPL bodies")
    return s2m


def smpl6d_qpos_device(full_6d, clip_start, models, clip_model=None, count_offset: bool = True, want=("qpos",), device=None):
    """6D rows -> qpos rows on the device (uhc_smpl6d_qpos): what `smpl_6d_to_qpose(clip, model)`, clip by clip, gives on the host.  The mirror of
    `smpl_qpos_device`: full_6d (n_frames, 147) = translation | 24 x (column 0, column 1 of the joint's rotation matrix); every other argument and the
    result as there."""
    if not torch.cuda.is_available():
        raise RuntimeError("uhc_amd.sim.smpl6d_qpos_device needs an MI355X (torch.cuda unavailable); there is no CPU fallback")
    ms = list(models) if isinstance(models, (list, tuple)) else [models]
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or len(set(want)) != len(want) or any(w not in ("qpos", "qpos_quat") for w in want):
        raise ValueError(f"smpl6d_qpos_device: want names 'qpos' and / or 'qpos_quat', got {want!r}")
    if device is None:
        device = full_6d.device if isinstance(full_6d, torch.Tensor) and full_6d.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    s2m = _smpl_table(ms, "smpl6d_qpos_device")
    full = torch.as_tensor(full_6d)
    n_frames = int(full.shape[0])
    if full.ndim != 2 or full.shape[1] != 147:
        raise ValueError(f"smpl6d_qpos_device: full_6d must be (n_frames, 147), got {tuple(full.shape)}")
    cs, cm = _clip_tables("smpl6d_qpos_device", clip_start, clip_model, n_frames, len(ms))
    widths = dict(qpos=76, qpos_quat=99)
    with torch.cuda.device(device):  # (the temporaries below are freed in stream order: the launch is on torch's current stream)
        out = {w: torch.empty((n_frames, widths[w]), dtype=torch.float64, device=device) for w in want}
        if n_frames:
            off = torch.from_numpy(np.stack([np.asarray(m.body_pos, dtype=np.float64)[1] for m in ms])).to(device).contiguous() if count_offset else None
            p = full.to(device, torch.float64).contiguous()
            d_cs = torch.from_numpy(cs.astype(np.int32)).to(device)
            d_cm = None if cm is None else torch.from_numpy(cm.astype(np.int32)).to(device)
            ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
            check(lib().uhc_smpl6d_qpos(C.c_void_p(torch.cuda.current_stream(device).cuda_stream), 24, s2m.ctypes.data_as(C.POINTER(C.c_int32)), ptr(off), len(ms),
                                        ptr(p), n_frames, ptr(d_cs), ptr(d_cm), int(cs.size), ptr(out.get("qpos")), ptr(out.get("qpos_quat"))))
    return tuple(out[w] for w in want)


POSE_WIDTHS = dict(pose_aa=72, trans=3, full_6d=147)


class SmplPoseOp:
    """What a `qpos_smpl_device` call needs of the models -- the joint table and the root offsets on the device -- kept, for callers that convert every
    control step (VecHumanoidEnv.smpl_pose): the call is then ONE launch, no upload and no allocation."""

    def __init__(self, models, device, count_offset=True):
        self.ms = list(models) if isinstance(models, (list, tuple)) else [models]
        self.device = torch.device(device)
        self.s2m = _smpl_table(self.ms, "qpos_smpl_device")
        self.ball = bool(int(self.ms[0].nq) != int(self.ms[0].nv) + 1)
        self.width = 99 if self.ball else 76
        self.off = torch.from_numpy(np.stack([np.asarray(m.body_pos, dtype=np.float64)[1] for m in self.ms])).to(self.device).contiguous() if count_offset else None
        self.bad = torch.zeros(1, dtype=torch.int32, device=self.device)

    def __call__(self, rows, n_seq, row_cap, seq_rows, seq_model, out, wait=False):
        """rows: a float64 device tensor whose rows of >= width doubles lie rows.stride(-2) apart; out: {name: contiguous tensor of n_seq * row_cap rows}"""
        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
        h_bad = C.c_int32(0)
        check(lib().uhc_qpos_smpl(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), 24, self.s2m.ctypes.data_as(C.POINTER(C.c_int32)), int(self.ball),
                                  ptr(self.off), len(self.ms), ptr(rows), int(rows.stride(-2)), int(n_seq), int(row_cap), ptr(seq_rows), ptr(seq_model),
                                  ptr(out.get("pose_aa")), ptr(out.get("trans")), ptr(out.get("full_6d")), ptr(self.bad), C.byref(h_bad) if wait else None))
        return int(h_bad.value) if wait else self.bad


def qpos_smpl_device(qpos, models, seq_rows=None, seq_model=None, count_offset: bool = True, want=("pose_aa", "trans"), out=None, wait=False):
    """qpos rows -> SMPL poses on the device (uhc_qpos_smpl): what `qpos_to_smpl(rows, model)` -- for the ball-joint humanoid `qpos_quat_to_smpl` -- gives
    on the host, from ONE launch on torch's current stream.
      qpos: (n_rows, w) or (n_seq, row_cap, w), float64 with unit inner stride; a device tensor is read where it lies, whatever its row stride (the
      simulation's qpos field with objects behind the humanoid, an evaluation record's pred_qpos, the qpos columns of the clip bank); anything else is uploaded.
      The rows are hinge rows (w >= 76) or, when the models are ball-joint models, ball-joint rows (w >= 99);
      models: one compiled `Model` (or a list of them, same body order) per body shape -- their root offsets (body_pos[1]) are subtracted from the root
      position when count_offset --, seq_model int32 (n_seq,) or None: which of them each sequence (each row of a 2-D qpos) is converted for; an entry out of
      range reads as 0; seq_rows int32 (n_seq,) or None: only the first seq_rows[s] rows (clamped to 0 .. row_cap) of sequence s are converted, every other
      output slot keeps what it held (NaN in a tensor made here);
      want: any of "pose_aa" (.., 72) in SMPL joint order, "trans" (.., 3), "full_6d" (.., 147) = trans | 24 x (column 0, column 1 of the rotation matrix);
      out: {name: tensor} to write into.
    Returns the float64 device tensors in the order of `want`, then `bad`: an int32 [1] device tensor, or -- wait=True, the call then waits for the stream --
    the int itself: the number of rows with a quaternion of zero or non-finite norm (scipy raises there); they are NaN throughout."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or len(set(want)) != len(want) or any(w not in POSE_WIDTHS for w in want):
        raise ValueError(f"qpos_smpl_device: want names 'pose_aa', 'trans' and / or 'full_6d', got {want!r}")
    if not torch.cuda.is_available():
        raise RuntimeError("uhc_amd.sim.qpos_smpl_device needs an MI355X (torch.cuda unavailable); there is no CPU fallback")
    device = qpos.device if isinstance(qpos, torch.Tensor) and qpos.is_cuda else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(device):
        op = SmplPoseOp(models, device, count_offset)
        rows = torch.as_tensor(qpos)
        if not (rows.is_cuda and rows.dtype == torch.float64):
            rows = rows.to(device, torch.float64).contiguous()
        if rows.ndim not in (2, 3) or rows.shape[-1] < op.width:
            raise ValueError(f"qpos_smpl_device: qpos must be (n_rows, >= {op.width}) or (n_seq, row_cap, >= {op.width}), got {tuple(rows.shape)}")
        n_seq, row_cap = (int(rows.shape[0]), 1) if rows.ndim == 2 else (int(rows.shape[0]), int(rows.shape[1]))
        lead = tuple(rows.shape[:-1])
        if rows.numel() and (rows.stride(-1) != 1 or (rows.ndim == 3 and rows.stride(0) != row_cap * rows.stride(1))):
            raise ValueError("qpos_smpl_device: qpos rows must have unit inner stride and lie one row stride apart")
        for name, t in (("seq_rows", seq_rows), ("seq_model", seq_model)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n_seq):
                raise ValueError(f"qpos_smpl_device: {name} must be a contiguous int32 device tensor of {n_seq} entries")
        res = {}
        for w in want:
            t = None if out is None else out.get(w)
            if t is None:
                t = torch.full(lead + (POSE_WIDTHS[w],), float("nan"), dtype=torch.float64, device=device)
            if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == n_seq * row_cap * POSE_WIDTHS[w]):
                raise ValueError(f"qpos_smpl_device: out[{w!r}] must be a contiguous float64 device tensor of {n_seq * row_cap} x {POSE_WIDTHS[w]}")
            res[w] = t
        if n_seq * row_cap == 0:
            return tuple(res[w] for w in want) + ((0 if wait else op.bad),)
        bad = op(rows, n_seq, row_cap, seq_rows, seq_model, res, wait=wait)
    return tuple(res[w] for w in want) + (bad,)


class EnvBatch:
    """Device env layer (uhc_env_* of the C-ABI) on top of a SimBatch."""

    def __init__(self, sim: SimBatch, desc: UhcEnvDesc):
        self.sim, self.L, self.desc = sim, sim.L, desc
        self._e = C.c_void_p()
        check(self.L.uhc_env_create(sim._b, C.byref(desc), C.byref(self._e)))
        self.obs_dim = self.L.uhc_env_obs_dim(self._e)
        self.n_env, self.device = sim.n_env, sim.device
        self._fields = {}
        self._bank = None

    def close(self):
        if getattr(self, "_e", None) is not None and self._e:
            if _capturing():
                _DEFERRED.append((self.L, "env", self._e, []))
                self._e = None
                return
            self.L.uhc_env_free(self._e)
            self._e = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def field(self, f: int) -> torch.Tensor:
        if f in self._fields:
            return self._fields[f]
        p, n = C.c_void_p(), C.c_int64()
        check(self.L.uhc_env_field(self._e, f, C.byref(p), C.byref(n)))
        per = n.value // self.n_env
        if f in _E_INT:
            t = torch.as_tensor(_DevView(p.value, (self.n_env,), "<i4", self), device=self.device)
        elif f in _E_ROWS:
            t = torch.as_tensor(_DevView(p.value, (_E_ROWS[f], self.n_env), "<f8", self), device=self.device)
        elif per == 1:
            t = torch.as_tensor(_DevView(p.value, (self.n_env,), "<f8", self), device=self.device)
        else:
            t = torch.as_tensor(_DevView(p.value, (self.n_env, per), "<f8", self), device=self.device)
        self._fields[f] = t
        return t

    generation = 0  # bumped whenever a device pointer the env kernels take BY VALUE changes (clip bank, clip -> model map): HIP graphs that
                    # captured env launches hold the old pointers and must be captured again (khrylib.rl.agents.Agent.rollout_step)

    def set_bank(self, frames: torch.Tensor, clip_start: torch.Tensor, clip_beta: torch.Tensor):
        self.generation += 1
        frames = frames.to(self.device, torch.float64).contiguous()
        clip_start = clip_start.to(self.device, torch.int32).contiguous()
        clip_beta = clip_beta.to(self.device, torch.float64).contiguous()
        assert frames.shape[1] == FRAME_STRIDE and clip_beta.shape == (clip_start.shape[0], 17)
        check(self.L.uhc_env_set_bank(self._e, C.c_void_p(frames.data_ptr()), frames.shape[0], C.c_void_p(clip_start.data_ptr()),
                                      C.c_void_p(clip_beta.data_ptr()), clip_start.shape[0]))
        self._bank = (frames, clip_start, clip_beta)  # keep alive: the library borrows the pointers
        self._live = None  # (a caller's bank ends live mode)

    def set_obj_pose(self, obj_pose: Optional[torch.Tensor]):
        """expert["obj_pose"] of every frame of the bank ([n_frames][7 num_obj]): where a reset puts the objects (humanoid_im.py:1284-1287)."""
        self.generation += 1
        if obj_pose is None:
            check(self.L.uhc_env_set_obj_pose(self._e, None, 0))
            self._obj_pose = None
            return
        op = obj_pose.to(self.device, torch.float64).contiguous()
        assert op.ndim == 2 and op.shape[0] == self._bank[0].shape[0] and op.shape[1] == 7 * int(self.desc.num_obj)
        check(self.L.uhc_env_set_obj_pose(self._e, C.c_void_p(op.data_ptr()), op.shape[0]))
        self._obj_pose = op  # borrowed by the library

    def set_clip_models(self, clip_model: Optional[torch.Tensor]):
        """Which of the batch's models the episodes of each clip run on (per-clip body shape); None switches it off."""
        self.generation += 1
        if clip_model is None:
            check(self.L.uhc_env_set_clip_models(self._e, None))
            self._clip_model = None
            return
        cm = clip_model.to(self.device, torch.int32).contiguous()
        assert cm.shape == (self._bank[1].shape[0],)
        check(self.L.uhc_env_set_clip_models(self._e, C.c_void_p(cm.data_ptr())))
        self._clip_model = cm  # borrowed by the library

    @staticmethod
    def _i32(t, device):
        return t.to(device, torch.int32).contiguous()

    def assign(self, env_ids, clip_ids, fr_start, fr_len):
        a, b, c, d = (self._i32(x, self.device) for x in (env_ids, clip_ids, fr_start, fr_len))
        check(self.L.uhc_env_assign(self._e, C.c_void_p(a.data_ptr()), a.shape[0], C.c_void_p(b.data_ptr()), C.c_void_p(c.data_ptr()),
                                    C.c_void_p(d.data_ptr())))

    def reset(self, env_ids, noise: Optional[torch.Tensor] = None):
        ids = self._i32(env_ids, self.device)
        nz = None
        if noise is not None:
            noise = noise.to(self.device, torch.float64).contiguous()
            assert noise.shape == (ids.shape[0], self.sim.model.nu)
            nz = C.c_void_p(noise.data_ptr())
        check(self.L.uhc_env_reset(self._e, C.c_void_p(ids.data_ptr()), ids.shape[0], nz))
        self._keep = (ids, noise)

    def set_next(self, env_ids, clip_ids, fr_start, fr_len, noise: Optional[torch.Tensor] = None):
        """Queue the window (and reset noise) the listed envs start when their current episode is done (uhc_env_set_next)."""
        a, b, c, d = (self._i32(x, self.device) for x in (env_ids, clip_ids, fr_start, fr_len))
        nz = None
        if noise is not None:
            noise = noise.to(self.device, torch.float64).contiguous()
            assert noise.shape == (a.shape[0], self.sim.model.nu)
            nz = C.c_void_p(noise.data_ptr())
        check(self.L.uhc_env_set_next(self._e, C.c_void_p(a.data_ptr()), a.shape[0], C.c_void_p(b.data_ptr()), C.c_void_p(c.data_ptr()),
                                      C.c_void_p(d.data_ptr()), nz))
        self._keep_next = (a, b, c, d, noise)  # alive until the stream has consumed them (the next call replaces them a step later)

    def set_next_host(self, env_ids, clip_ids, fr_start, fr_len, noise=None):
        """set_next from host (numpy) arrays: the five arrays are packed into one buffer and go down in ONE copy (a copy from pageable
        memory waits for everything queued before it; five of them per control step cost ~0.1 ms of idle GPU).  Measured alternatives,
        both dropped: an asynchronous copy from a pinned ring, and the kernel reading the pinned buffer over PCIe itself -- with either
        the host runs ahead of the GPU and the step time became erratic (4.1 .. 8 ms against a steady 4.1)."""
        import numpy as np
        k, nu = int(len(env_ids)), self.sim.model.nu
        if k == 0:
            return
        nbytes = 16 * k + (8 * k * nu if noise is not None else 0)
        hb = np.empty(nbytes, dtype=np.uint8)
        ints = hb[:16 * k].view(np.int32).reshape(4, k)
        ints[0], ints[1], ints[2], ints[3] = env_ids, clip_ids, fr_start, fr_len
        if noise is not None:
            hb[16 * k:].view(np.float64).reshape(k, nu)[...] = noise
        dev = self.__dict__.get("_next_dev")
        if dev is None or dev.numel() < nbytes:
            dev = self._next_dev = torch.empty(max(nbytes, 16 * self.n_env + 8 * self.n_env * nu), dtype=torch.uint8, device=self.device)
        dev[:nbytes].copy_(torch.from_numpy(hb))
        base = dev.data_ptr()
        check(self.L.uhc_env_set_next(self._e, C.c_void_p(base), k, C.c_void_p(base + 4 * k), C.c_void_p(base + 8 * k), C.c_void_p(base + 12 * k),
                                      C.c_void_p(base + 16 * k) if noise is not None else None))

    def auto_reset(self):
        """Device-side episode turnover of every env whose done flag is set (uhc_env_auto_reset); no host round trip."""
        check(self.L.uhc_env_auto_reset(self._e))

    def set_end_reward(self, v: float):
        check(self.L.uhc_env_set_end_reward(self._e, float(v)))

    # ---- live targets (uhc_env_live_*): each env imitates a stream of frames appended while it runs
    def live_begin(self, cap: int, humanoids, beta: Optional[torch.Tensor] = None, dt: float = 1 / 30):
        """Give every env a stream of up to `cap` frames in a bank the LIBRARY owns (n_env x cap x 4 672 B) and make it the env's clip bank.
          humanoids: one `Humanoid` (or a list, same tree) per model of the batch -- their offset tables are copied --; beta (n_env, 17) or None (zeros):
          what has_shape observations append.  Every stream starts empty: `live_push(..., restart=1)` its frame 0, push on, then `reset`."""
        hs = list(humanoids) if isinstance(humanoids, (list, tuple)) else [humanoids]
        parents = np.ascontiguousarray(hs[0]._parents, dtype=np.int32)
        ee = np.ascontiguousarray(hs[0]._ee_idx, dtype=np.int32)
        for h in hs[1:]:
            if not np.array_equal(np.asarray(h._parents), parents) or list(h._ee_idx) != list(ee):
                raise ValueError("live_begin: every body shape must share the first one's tree")
        if ee.shape != (5,):
            raise ValueError("live_begin: five end effectors (SMPL_EE_NAMES) are what the frame record holds")
        self.generation += 1
        off = torch.stack([h._offsets for h in hs]).to(self.device, torch.float64).contiguous()
        ioff = torch.stack([h._i_offsets for h in hs]).to(self.device, torch.float64).contiguous()
        b = None
        if beta is not None:
            b = torch.as_tensor(beta).to(self.device, torch.float64).contiguous()
            if tuple(b.shape) != (self.n_env, 17):
                raise ValueError(f"live_begin: beta must be ({self.n_env}, 17), got {tuple(b.shape)}")
        torch.cuda.current_stream(self.device).synchronize()  # (the tables above are copied by the call, on the library's side)
        check(self.L.uhc_env_live_begin(self._e, int(cap), int(off.shape[1]), parents.ctypes.data_as(C.POINTER(C.c_int32)), ee.ctypes.data_as(C.POINTER(C.c_int32)),
                                        C.c_void_p(off.data_ptr()), C.c_void_p(ioff.data_ptr()), len(hs), float(dt), None if b is None else C.c_void_p(b.data_ptr())))
        self._bank = None
        self._live = None

    def live_push(self, env_ids, qpos, restart=None, root_quat_record=None, model=None):
        """One row (76 wide, as `expert_frames_device` takes them) per listed env, appended to its stream -- or, where restart != 0, frame 0 of a new
        one (on `model`'s body shape, when given) --: ONE launch, no host read; device tensors of the right type are taken as they are, so the call can
        be captured into a graph.  Each env at most once per call.  A row for an env without a stream, or with a full one, is counted in `dropped`."""
        ids = self._i32(torch.as_tensor(env_ids), self.device)
        q = torch.as_tensor(qpos).to(self.device, torch.float64).contiguous()
        n = int(ids.shape[0])
        if ids.ndim != 1 or tuple(q.shape) != (n, 76):
            raise ValueError(f"live_push: env_ids (n,) and qpos (n, 76) expected, got {tuple(ids.shape)} and {tuple(q.shape)}")
        rq = None if root_quat_record is None else torch.as_tensor(root_quat_record).to(self.device, torch.float64).contiguous()
        if rq is not None and tuple(rq.shape) != (n, 4):
            raise ValueError(f"live_push: root_quat_record must be ({n}, 4), got {tuple(rq.shape)}")
        rs = None if restart is None else self._i32(torch.as_tensor(restart), self.device)
        md = None if model is None else self._i32(torch.as_tensor(model), self.device)
        for name, t in (("restart", rs), ("model", md)):
            if t is not None and tuple(t.shape) != (n,):
                raise ValueError(f"live_push: {name} must be ({n},), got {tuple(t.shape)}")
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        check(self.L.uhc_env_live_push(self._e, ptr(ids), n, ptr(q), ptr(rq), ptr(rs), ptr(md)))
        self._keep_live = (ids, q, rq, rs, md)  # alive until the stream has consumed them (the next call replaces them a step later)

    def live_view(self):
        """(frames (n_env, cap, FRAME_STRIDE), len (n_env,), dropped (n_env,)): zero-copy torch views of the live bank and its counters."""
        if getattr(self, "_live", None) is None:
            pf, pl, pd, cap = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int32()
            check(self.L.uhc_env_live_view(self._e, C.byref(pf), C.byref(pl), C.byref(pd), C.byref(cap)))
            self._live = (torch.as_tensor(_DevView(pf.value, (self.n_env, cap.value, FRAME_STRIDE), "<f8", self), device=self.device),
                          torch.as_tensor(_DevView(pl.value, (self.n_env,), "<i4", self), device=self.device),
                          torch.as_tensor(_DevView(pd.value, (self.n_env,), "<i4", self), device=self.device))
        return self._live

    def live_slide(self, on: bool = True):
        """Endless streams (uhc_env_live_slide; `live_begin` switches it off): from now on `live_push` makes room before it appends -- where a listed env's
        stream is full, the records behind the frame the env reads next are discarded and the others move to the front of its slice, on the device, in the
        same call.  The env is driven exactly as by a stream that never slid; `E_PERCENT` is then cur_t / (len - 1) of the window, not a progress measure.
        Refused outside live mode and for observation v0 with the phase word."""
        check(self.L.uhc_env_live_slide(self._e, 1 if on else 0))

    def live_window(self):
        """(base (n_env,), moved (n_env,)): zero-copy int32 views.  base: frames slid off since the restart -- slot i of `live_view()[0]` holds global frame
        base + i, and base + len frames were accepted --; moved: records copied by slides since the restart."""
        if getattr(self, "_live_win", None) is None or self._live_win[0] != self.generation:
            pb, pm = C.c_void_p(), C.c_void_p()
            check(self.L.uhc_env_live_window(self._e, C.byref(pb), C.byref(pm)))
            self._live_win = (self.generation, torch.as_tensor(_DevView(pb.value, (self.n_env,), "<i4", self), device=self.device),
                              torch.as_tensor(_DevView(pm.value, (self.n_env,), "<i4", self), device=self.device))
        return self._live_win[1:]

    def live_end(self):
        """Leave live mode: the env has no bank until the next `set_bank` / `live_begin` (the live memory stays the env's)."""
        self.generation += 1
        check(self.L.uhc_env_live_end(self._e))
        self._live = None

    def step(self, action: torch.Tensor, active: Optional[torch.Tensor] = None):
        assert action.dtype == torch.float64 and action.is_contiguous() and action.shape == (self.n_env, self.sim.ctrl.action_dim)
        a = None
        if active is not None:
            assert active.dtype == torch.int32 and active.is_contiguous()
            a = C.c_void_p(active.data_ptr())
        check(self.L.uhc_env_step(self._e, C.c_void_p(action.data_ptr()), a))


def make_ctrl(model, *, meta_pd: bool = True, meta_pd_joint: bool = False, residual_force: bool = True,
              residual_force_mode: str = "implicit", residual_force_scale: float = 100.0, residual_force_lim: float = 100.0,
              rfc_rate: float = 1.0, action_type: str = "position", pd_mul: float = 1.0, tq_mul: float = 1.0,
              base_rot=(0.7071, 0.7071, 0.0, 0.0), n_substeps: int = 15, residual_force_bodies="all",
              residual_force_torque: bool = True) -> UhcCtrlDesc:
    """UhcCtrlDesc from the reference's config knobs (copycat_config.py:86-113, humanoid_im.py:120-124,226-255)."""
    from ._capi import ctrl_desc
    from .smpllib.smpl_mujoco import SMPLConverter

    conv = SMPLConverter(model, model)
    nu = model.nu
    rfc_mode = 0
    vf_dim = 0
    vf_body, body_vf_dim, scale = None, 9, residual_force_scale * rfc_rate
    if residual_force:
        if residual_force_mode == "implicit":
            rfc_mode, vf_dim = 1, 6
        else:  # explicit: one (contact point, force[, torque]) per body, bodies in SMPL joint order (humanoid_im.py:236-243)
            from .smpllib.smpl_mujoco import SMPL_BONE_ORDER_NAMES
            names = SMPL_BONE_ORDER_NAMES if residual_force_bodies == "all" else list(residual_force_bodies)
            vf_body = [model.body_names.index(n) for n in names]
            body_vf_dim = 6 + 3 * int(bool(residual_force_torque))
            rfc_mode, vf_dim, scale = 2, body_vf_dim * len(vf_body), residual_force_scale  # rfc_explicit does not apply rfc_rate
    mp = 1 if meta_pd else (2 if meta_pd_joint else 0)
    mp_dim = 2 * n_substeps if mp == 1 else (2 * nu if mp == 2 else 0)
    return ctrl_desc(n_substeps=n_substeps, action_type=0 if action_type == "position" else 1, meta_pd=mp, rfc_mode=rfc_mode,
                     action_dim=nu + vf_dim + mp_dim, rfc_scale=scale, rfc_lim=residual_force_lim, vf_body=vf_body, body_vf_dim=body_vf_dim,
                     base_rot=base_rot, jkp=conv.get_new_jkp() * pd_mul, jkd=conv.get_new_jkd() * pd_mul,
                     torque_lim=conv.get_new_torque_limit() * tq_mul, a_scale=conv.get_new_a_scale())


def load_asset_model(name: str = "humanoid_smpl_neutral_mesh"):
    import os
    from .model.mjcf import Model
    return Model.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets", name + ".npz"))
