"""Host side of the evaluation kernels (uhc_amd/csrc/uhc_eval.hip; C-ABI in include/uhc_amd.h): thin ctypes calls on torch tensors, like rollout_ops.
The record of an episode batch -- what eval_seqs reads out per control step -- lives in torch tensors the caller owns (Record); uhc_eval_record appends
to it on the device, uhc_eval_metrics scores it against the clip bank.  Device float64 / int32 / int64 only; there is no CPU path."""
import ctypes as C

import torch

from ._lib import check, lib

N_BODY = 24
METRICS = ("root_dist", "vel_dist", "accel_dist", "mpjpe_g", "pa_mpjpe", "mpjpe")  # the order of a row of row_metrics (uhc_eval_metrics.h)
SURFACE_METRICS = ("pentration", "skate", "float", "contact")  # the order of a row of uhc_surface_metrics' output (uhc_surface_math.h); the reference's spelling
POSE_ROW, POSE_QUAT = 7 * N_BODY, 3 * N_BODY  # a pose record's row: 72 position doubles, then 96 quaternion doubles
FRAME_STRIDE, FR_WBPOS, FR_WBQUAT = 584, 151, 223  # the clip bank's frame record (include/uhc_amd.h, uhc_device_env.h)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class Record:
    """The caller-owned state of uhc_eval_record for n_env envs, zeroed: up to row_cap rows per env."""

    def __init__(self, n_env, row_cap, nqh, device, poses=False):
        z = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device=device)
        # poses: the record also keeps xpos / xquat of bodies 1 .. 24 per row (record_pose), what the surface metrics read
        self.pred_pose = z(n_env, row_cap, POSE_ROW) if poses else None
        self.n_env, self.row_cap, self.nqh = int(n_env), int(row_cap), int(nqh)
        self.rows, self.steps = z(n_env, dtype=torch.int32), z(n_env, dtype=torch.int32)
        self.pred_qpos, self.pred_jpos = z(n_env, row_cap, nqh), z(n_env, row_cap, 3 * N_BODY)
        self.gt_frame = z(n_env, row_cap, dtype=torch.int64)
        self.rewards = z(n_env, row_cap)
        self.fail_safe, self.percent, self.tele = z(n_env, dtype=torch.int32), z(n_env), z(n_env, dtype=torch.int32)
        self.overflow = z(1, dtype=torch.int32)


def record(rec, phase, t, qpos, xpos, clip0, lens, alive, done=None, reward=None, percent=None, fail_safe=False):
    """One snapshot of the envs with alive != 0: phase 0 before the step, phase 1 after it (done / reward / percent: the step's outputs).
    qpos [n_env][nq], xpos [n_env][3 nbody] (body 0 = the world): the simulation's own fields; clip0 int64 / lens int32 [n_env]: first bank frame and
    length of each env's clip; alive int32 [n_env]: the mask handed to the env step -- phase 1 clears the entries of finished episodes."""
    n_env = rec.n_env
    assert qpos.dtype == xpos.dtype == torch.float64 and qpos.is_contiguous() and xpos.is_contiguous() and qpos.shape[0] == xpos.shape[0] == n_env
    assert clip0.dtype == torch.int64 and lens.dtype == torch.int32 and alive.dtype == torch.int32 and clip0.numel() == lens.numel() == alive.numel() == n_env
    assert clip0.is_contiguous() and lens.is_contiguous() and alive.is_contiguous() and xpos.shape[1] % 3 == 0
    if phase == 1:
        assert done.dtype == torch.int32 and reward.dtype == percent.dtype == torch.float64 and done.numel() == reward.numel() == percent.numel() == n_env
        assert done.is_contiguous() and reward.is_contiguous() and percent.is_contiguous()
    check(lib().uhc_eval_record(_stream(qpos), int(phase), n_env, N_BODY, qpos.shape[1], rec.nqh, xpos.shape[1] // 3, rec.row_cap, int(t), int(bool(fail_safe)),
                                _p(qpos), _p(xpos), _p(clip0), _p(lens), _p(done), _p(reward), _p(percent), _p(alive), _p(rec.rows), _p(rec.steps),
                                _p(rec.pred_qpos), _p(rec.pred_jpos), _p(rec.gt_frame), _p(rec.rewards), _p(rec.fail_safe), _p(rec.percent), _p(rec.tele),
                                _p(rec.overflow)))


def metrics(rec, frames, row_metrics=None, clip_means=None, wait=False):
    """compute_metrics of every env of the record against the bank `frames` [n_frames][FRAME_STRIDE] -> (row_metrics [n_env][row_cap][6], clip_means
    [n_env][6], bad): METRICS order, mm; slots beyond an env's rows (rows - 1 for vel_dist, rows - 2 for accel_dist) keep what they held (NaN in a tensor
    made here).  bad: an int32 [1] device tensor, or -- wait=True, the call then waits for the stream -- the int itself: how many gt_frame entries lay
    outside the bank (the outputs that would have read them are NaN)."""
    assert frames.dtype == torch.float64 and frames.is_contiguous() and frames.dim() == 2
    dev = frames.device
    if row_metrics is None:
        row_metrics = torch.full((rec.n_env, rec.row_cap, len(METRICS)), float("nan"), dtype=torch.float64, device=dev)
    if clip_means is None:
        clip_means = torch.empty(rec.n_env, len(METRICS), dtype=torch.float64, device=dev)
    assert row_metrics.is_contiguous() and row_metrics.shape == (rec.n_env, rec.row_cap, len(METRICS)) and clip_means.is_contiguous()
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    h_bad = C.c_int32(0)
    check(lib().uhc_eval_metrics(_stream(frames), rec.n_env, N_BODY, rec.nqh, rec.row_cap, _p(rec.rows), _p(rec.pred_qpos), _p(rec.pred_jpos), _p(rec.gt_frame),
                                 _p(frames), frames.shape[0], _p(row_metrics), _p(clip_means), _p(bad), C.byref(h_bad) if wait else None))
    return row_metrics, clip_means, (int(h_bad.value) if wait else bad)


def record_pose(rec, phase, xpos, xquat, alive, done=None):
    """The body poses of the snapshot `record` is about to take: xpos [n_env][3 nbody], xquat [n_env][4 nbody] (the simulation's own fields) of bodies
    1 .. 24 into row rec.rows[e] of rec.pred_pose, for the envs record's own rule selects.  It reads rec.rows and leaves it alone: call it directly BEFORE
    record(...) of the same snapshot, on the same stream."""
    if rec.pred_pose is None:
        raise ValueError("record_pose: the record keeps no poses (Record(..., poses=True))")
    n_env = rec.n_env
    assert xpos.dtype == xquat.dtype == torch.float64 and xpos.is_contiguous() and xquat.is_contiguous() and xpos.shape[0] == xquat.shape[0] == n_env
    assert xpos.shape[1] % 3 == 0 and xquat.shape[1] == xpos.shape[1] // 3 * 4
    assert alive.dtype == torch.int32 and alive.is_contiguous() and alive.numel() == n_env
    if phase == 1:
        assert done.dtype == torch.int32 and done.is_contiguous() and done.numel() == n_env
    check(lib().uhc_eval_record_pose(_stream(xpos), int(phase), n_env, xpos.shape[1] // 3, rec.row_cap, _p(xpos), _p(xquat), _p(done), _p(alive), _p(rec.rows),
                                     _p(rec.pred_pose)))


class Surface:
    """The hull vertices of one or several compiled models that share a topology (the humanoid's bodies 1 .. body_lim - 1, the geoms that own vertices:
    smpl_eval.surface_tables), on the current device: what uhc_surface_metrics scores poses against.  models: a compiled model, a list of them (index =
    the clip's body shape), or a list of surface_tables() triples (vert, vert_body, vert_radius).  n_body: the bodies of a pose row (default: 24 for
    compiled models, the largest body of the triples + 1)."""

    def __init__(self, models, body_lim=N_BODY + 1, n_body=None):
        import numpy as np
        from .smpllib.smpl_eval import surface_tables
        models = list(models) if isinstance(models, (list, tuple)) else [models]
        if not models:
            raise ValueError("Surface: no model")
        compiled = not isinstance(models[0], tuple)
        tabs = [surface_tables(m, body_lim) if compiled else m for m in models]
        vert, body, radius = tabs[0]
        for i, (v, b, r) in enumerate(tabs[1:], 1):
            if v.shape != vert.shape:
                raise ValueError(f"Surface: model {i} has {v.shape[0]} hull vertices, model 0 has {vert.shape[0]} (one topology expected)")
            if not (np.array_equal(b, body) and np.array_equal(r, radius)):  # (the device keeps ONE body and ONE radius table)
                raise ValueError(f"Surface: model {i} deals its vertices to other bodies, or with other radii, than model 0")
        self.n_body = int(n_body if n_body is not None else (body_lim - 1 if compiled else int(body.max()) + 1))
        self.n_vert, self.n_models = int(vert.shape[0]), len(tabs)
        self.tables = tabs  # (host copies: what hull_vertices takes)
        vb = np.ascontiguousarray(body, dtype=np.int32)
        vr = np.ascontiguousarray(radius, dtype=np.float64)
        vv = np.ascontiguousarray(np.stack([t[0] for t in tabs]), dtype=np.float64)
        h = C.c_void_p()
        self._L = lib()
        check(self._L.uhc_surface_create(self.n_body, self.n_vert, self.n_models, vb.ctypes.data_as(C.c_void_p), vr.ctypes.data_as(C.c_void_p),
                                         vv.ctypes.data_as(C.c_void_p), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.uhc_surface_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def surface_metrics(surface, pos, quat, seq_start, seq_rows, row_cap=None, seq_model=None, floor_z=0.0, row_out=None, seq_means=None, wait=False):
    """Penetration, skate, float and contact count of sequences of body poses -> (row_out [n_rows_total][4], seq_means [n_seq][4], bad): SURFACE_METRICS
    order, mm.  pos [n_rows_total][>= 3 n_body], quat [n_rows_total][>= 4 n_body]: 2-D float64 views with unit inner stride -- columns of a pose record
    or of the clip bank, read where they lie (their row strides travel); seq_start int64 / seq_rows int32 [n_seq]: first global row and row count of
    each sequence (clamped to 0 .. row_cap; row_cap None: max(seq_rows), which reads it back); seq_model int32 [n_seq] or None.  Slots of row_out that
    belong to no row of a sequence keep what they held (NaN in a tensor made here).  bad: an int32 [1] device tensor, or -- wait=True, the call then
    waits for the stream -- the int itself: rows with a non-finite pose (their values are NaN) plus sequences outside the rows (skipped)."""
    assert pos.dtype == quat.dtype == torch.float64 and pos.dim() == quat.dim() == 2 and pos.shape[0] == quat.shape[0]
    assert pos.stride(1) == 1 and quat.stride(1) == 1 and pos.shape[1] >= 3 * surface.n_body and quat.shape[1] >= 4 * surface.n_body
    assert seq_start.dtype == torch.int64 and seq_rows.dtype == torch.int32 and seq_start.is_contiguous() and seq_rows.is_contiguous()
    n_seq, n_rows = seq_start.numel(), pos.shape[0]
    assert seq_rows.numel() == n_seq and (seq_model is None or (seq_model.dtype == torch.int32 and seq_model.is_contiguous() and seq_model.numel() == n_seq))
    dev = pos.device
    if row_cap is None:
        row_cap = max(int(seq_rows.max().item()), 1) if n_seq else 1
    if row_out is None:
        row_out = torch.full((n_rows, len(SURFACE_METRICS)), float("nan"), dtype=torch.float64, device=dev)
    if seq_means is None:
        seq_means = torch.full((n_seq, len(SURFACE_METRICS)), float("nan"), dtype=torch.float64, device=dev)
    assert row_out.is_contiguous() and row_out.numel() >= n_rows * len(SURFACE_METRICS) and seq_means.is_contiguous() and seq_means.numel() >= n_seq * len(SURFACE_METRICS)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    h_bad = C.c_int32(0)
    check(lib().uhc_surface_metrics(_stream(pos), surface._h, n_seq, _p(seq_start), _p(seq_rows), int(row_cap), _p(seq_model), _p(pos), pos.stride(0), _p(quat),
                                    quat.stride(0), n_rows, float(floor_z), _p(row_out), _p(seq_means), _p(bad), C.byref(h_bad) if wait else None))
    return row_out, seq_means, (int(h_bad.value) if wait else bad)


def surface_metrics_of_record(surface, rec, seq_model=None, **kw):
    """surface_metrics of every env of a record that keeps poses: sequence e = the rows 0 .. rec.rows[e] - 1 of env e.
    -> (row_out [n_env][row_cap][4], seq_means [n_env][4], bad)"""
    if rec.pred_pose is None:
        raise ValueError("surface_metrics_of_record: the record keeps no poses (Record(..., poses=True))")
    flat = rec.pred_pose.view(rec.n_env * rec.row_cap, POSE_ROW)
    start = torch.arange(rec.n_env, dtype=torch.int64, device=flat.device) * rec.row_cap
    row_out, means, bad = surface_metrics(surface, flat[:, :POSE_QUAT], flat[:, POSE_QUAT:], start, rec.rows, row_cap=rec.row_cap, seq_model=seq_model, **kw)
    return row_out.view(rec.n_env, rec.row_cap, len(SURFACE_METRICS)), means, bad


def smpl_of_record(rec, models, seq_model=None, want=("pose_aa", "trans"), wait=False):
    """The recorded motion of every env as SMPL parameters (uhc_qpos_smpl, sim.qpos_smpl_device): rec.pred_qpos is read where it lies, rec.rows are the row
    counts.  models: the compiled model(s) of the humanoid (hinge or ball-joint), seq_model int32 [n_env] or None: each env's body shape.
    -> the tensors of `want` ([n_env][row_cap][72 / 3 / 147]; slots beyond an env's rows are NaN), then bad as qpos_smpl_device returns it."""
    from .sim import qpos_smpl_device
    return qpos_smpl_device(rec.pred_qpos, models, seq_rows=rec.rows, seq_model=seq_model, want=want, wait=wait)


def smpl_of_bank(frames, clip_start, models, clip_model=None, want=("pose_aa", "trans"), wait=False):
    """The expert clips themselves as SMPL parameters, from the qpos columns of the bank (hinge rows: the bank of the ball-joint humanoid keeps its joint
    quaternions elsewhere and is not served).  frames [n_frames][FRAME_STRIDE]; clip_start [n_clips] (any integer tensor or sequence, ascending from 0) and
    clip_model [n_clips] or None: which body shape's root offset a clip's frames lose.  -> the tensors of `want` ([n_frames][72 / 3 / 147]), then bad."""
    from .sim import qpos_smpl_device
    assert frames.dtype == torch.float64 and frames.dim() == 2 and frames.shape[1] == FRAME_STRIDE and frames.is_contiguous()
    ms = list(models) if isinstance(models, (list, tuple)) else [models]
    if int(ms[0].nq) != int(ms[0].nv) + 1:
        raise NotImplementedError("smpl_of_bank: the bank's qpos columns are hinge rows; the ball-joint humanoid's joint quaternions are not among them")
    dev = frames.device
    row_model = None
    if clip_model is not None and frames.shape[0]:  # every frame is a sequence of one row: the frame's model is its clip's
        start = torch.as_tensor(clip_start).to(dev, torch.int64).contiguous()
        clip_of = torch.searchsorted(start, torch.arange(frames.shape[0], device=dev), right=True) - 1
        row_model = torch.as_tensor(clip_model).to(dev, torch.int32)[clip_of.clamp_(0, start.numel() - 1)].contiguous()
    return qpos_smpl_device(frames[:, 0:76], ms, seq_model=row_model, want=want, wait=wait)


def surface_metrics_of_bank(surface, frames, clip_start, clip_len, clip_model=None, **kw):
    """surface_metrics of the expert clips themselves: frames [n_frames][FRAME_STRIDE] (the clip bank), clip_start / clip_len [n_clips] (any integer
    tensors or sequences), clip_model [n_clips] or None.  -> (row_out [n_frames][4], clip_means [n_clips][4], bad)"""
    assert frames.dtype == torch.float64 and frames.dim() == 2 and frames.shape[1] == FRAME_STRIDE and frames.is_contiguous()
    dev = frames.device
    start = torch.as_tensor(clip_start).to(dev, torch.int64).contiguous()
    rows = torch.as_tensor(clip_len).to(dev, torch.int32).contiguous()
    model = None if clip_model is None else torch.as_tensor(clip_model).to(dev, torch.int32).contiguous()
    return surface_metrics(surface, frames[:, FR_WBPOS:FR_WBPOS + 3 * N_BODY], frames[:, FR_WBQUAT:FR_WBQUAT + 4 * N_BODY], start, rows, seq_model=model, **kw)


# ------------------------------------------------------------------ the SMPL body mesh (uhc_amd/csrc/uhc_smpl_mesh.hip)
MESH_WANT = ("vertices", "joints", "metrics", "rows", "means", "zmin")


class SmplMesh:
    """The tables of one or several SMPL models (smpllib.smpl_mesh.load_smpl_model: the genders; they share the vertex count and the joint tree) on the
    current device, in the layout uhc_smpl_mesh reads.  The handle also owns what a call keeps between its kernels: use it on one stream at a time.  A call
    with more sequences (or, for means without rows, more rows) than any before it frees and allocates that space inside the call, so it cannot be
    captured into a graph; a first call of the largest shape outside the capture settles it."""

    def __init__(self, models):
        import numpy as np
        models = list(models) if isinstance(models, (list, tuple)) else [models]
        if not models:
            raise ValueError("SmplMesh: no model")
        V = int(models[0]["v_template"].shape[0])
        for i, m in enumerate(models[1:], 1):
            if m["v_template"].shape[0] != V:
                raise ValueError(f"SmplMesh: model {i} has {m['v_template'].shape[0]} vertices, model 0 has {V} (one topology expected)")
            if not np.array_equal(m["parents"], models[0]["parents"]):
                raise ValueError(f"SmplMesh: model {i} has another joint tree than model 0")
        self.n_vert, self.n_models, self.models = V, len(models), models
        stack = lambda k: np.ascontiguousarray(np.stack([np.asarray(m[k], dtype=np.float64) for m in models]))
        tabs = [stack(k) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")]
        parents = np.ascontiguousarray(models[0]["parents"], dtype=np.int32)
        h = C.c_void_p()
        self._L = lib()
        check(self._L.uhc_smpl_mesh_create(V, self.n_models, *[t.ctypes.data_as(C.c_void_p) for t in tabs], parents.ctypes.data_as(C.c_void_p), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.uhc_smpl_mesh_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def smpl_mesh(mesh, pose_aa, trans, seq_start, seq_rows, betas, seq_model=None, want=("metrics",), floor_z=0.0, wait=False, row_cap=None, out=None):
    """Posed SMPL bodies on the device -> {name: tensor} for the names of `want` plus "bad":
      "vertices" [n_rows][V][3], "joints" [n_rows][24][3], "rows" -> "row_out" [n_rows][4] and "means" -> "seq_means" [n_seq][4] (SURFACE_METRICS order, mm,
      on SMPL vertices; "metrics" asks for both), "zmin" [n_rows]: the lowest vertex z of each row.
    pose_aa [n_rows][>= 72], trans [n_rows][>= 3]: 2-D float64 device views with unit inner stride, read where they lie (qpos_smpl_device's outputs flattened
    over their leading dimensions); seq_start int64 / seq_rows int32 [n_seq] as for surface_metrics (row_cap None: max(seq_rows), which reads it back);
    betas float64 [n_seq][10]; seq_model int32 [n_seq] or None: which of the mesh's models (genders) a sequence is.  Slots of rows outside every sequence
    keep what they held (NaN in a tensor made here; `out`: {key: tensor} to write into).  bad: an int32 [1] device tensor, or -- wait=True, the call then
    waits for the stream -- the int itself: rows with a non-finite pose or translation (NaN throughout) plus sequences outside the rows (skipped)."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in MESH_WANT for w in want):
        raise ValueError(f"smpl_mesh: want names any of {MESH_WANT}, got {want!r}")
    assert pose_aa.dtype == trans.dtype == betas.dtype == torch.float64 and pose_aa.dim() == trans.dim() == 2 and pose_aa.shape[0] == trans.shape[0]
    assert (pose_aa.numel() == 0 or pose_aa.stride(1) == 1) and (trans.numel() == 0 or trans.stride(1) == 1) and pose_aa.shape[1] >= 3 * N_BODY and trans.shape[1] >= 3
    assert seq_start.dtype == torch.int64 and seq_rows.dtype == torch.int32 and seq_start.is_contiguous() and seq_rows.is_contiguous()
    n_seq, n_rows, dev = seq_start.numel(), pose_aa.shape[0], pose_aa.device
    assert seq_rows.numel() == n_seq and (seq_model is None or (seq_model.dtype == torch.int32 and seq_model.is_contiguous() and seq_model.numel() == n_seq))
    assert betas.is_contiguous() and betas.shape == (n_seq, 10)
    if row_cap is None:
        row_cap = max(int(seq_rows.max().item()), 1) if n_seq else 1
    shapes = {"vertices": (n_rows, mesh.n_vert, 3), "joints": (n_rows, N_BODY, 3), "row_out": (n_rows, len(SURFACE_METRICS)), "seq_means": (n_seq, len(SURFACE_METRICS)),
              "zmin": (n_rows,)}
    keys = [k for k, on in (("vertices", "vertices" in want), ("joints", "joints" in want), ("row_out", "metrics" in want or "rows" in want),
                            ("seq_means", "metrics" in want or "means" in want), ("zmin", "zmin" in want)) if on]
    res = {}
    for k in keys:
        t = None if out is None else out.get(k)
        if t is None:
            t = torch.full(shapes[k], float("nan"), dtype=torch.float64, device=dev)
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shapes[k], k
        res[k] = t
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    if n_seq == 0:  # nothing to launch (and empty tensors have no address to hand over)
        res["bad"] = 0 if wait else bad
        return res
    h_bad = C.c_int32(0)
    ps, ts = (pose_aa.stride(0) if n_rows > 1 else pose_aa.shape[1]), (trans.stride(0) if n_rows > 1 else trans.shape[1])
    check(lib().uhc_smpl_mesh(_stream(pose_aa), mesh._h, n_seq, _p(seq_start), _p(seq_rows), int(row_cap), _p(seq_model), _p(betas), _p(pose_aa), ps, _p(trans), ts,
                              n_rows, float(floor_z), _p(res.get("vertices")), _p(res.get("joints")), _p(res.get("row_out")), _p(res.get("seq_means")),
                              _p(res.get("zmin")), _p(bad), C.byref(h_bad) if wait else None))
    res["bad"] = int(h_bad.value) if wait else bad
    return res


def _mesh_seq(betas, seq_gender, n_seq, dev):
    b = torch.as_tensor(betas).to(dev, torch.float64).reshape(-1, torch.as_tensor(betas).shape[-1])[:, :10]
    b = (b.expand(n_seq, 10) if b.shape[0] == 1 else b).contiguous()
    g = None if seq_gender is None else torch.as_tensor(seq_gender).to(dev, torch.int32).contiguous()
    return b, g


def mesh_metrics_of_record(mesh, rec, models, betas, seq_model=None, seq_gender=None, want=("metrics",), **kw):
    """The contact quality of every env's recorded motion on SMPL vertices: smpl_of_record (rec.pred_qpos -> pose_aa, trans on the device), then smpl_mesh
    on them where they lie -- no pose leaves the device.  models / seq_model: the compiled humanoid model(s) and each env's body shape, as for
    smpl_of_record; betas [n_env][10 | 16] (or one row for all) and seq_gender [n_env] or None: each env's SMPL shape and which of the mesh's models it is.
    -> smpl_mesh's dict, the row tensors as [n_env][row_cap][...]; "bad" adds the rows smpl_of_record found bad when both are counts (wait=True)."""
    pose_aa, trans, bad0 = smpl_of_record(rec, models, seq_model=seq_model, wait=bool(kw.get("wait", False)))
    n, dev = rec.n_env * rec.row_cap, pose_aa.device
    b, g = _mesh_seq(betas, seq_gender, rec.n_env, dev)
    start = torch.arange(rec.n_env, dtype=torch.int64, device=dev) * rec.row_cap
    res = smpl_mesh(mesh, pose_aa.view(n, 72), trans.view(n, 3), start, rec.rows, b, seq_model=g, want=want, row_cap=rec.row_cap, **kw)
    for k in ("vertices", "joints", "row_out", "zmin"):
        if k in res:
            res[k] = res[k].view((rec.n_env, rec.row_cap) + tuple(res[k].shape[1:]))
    res["bad"] = res["bad"] + bad0
    return res


def mesh_metrics_of_bank(mesh, frames, clip_start, clip_len, models, betas, clip_model=None, clip_gender=None, want=("metrics",), **kw):
    """The counterpart for the expert clips themselves: smpl_of_bank on the bank's qpos columns (hinge rows), then smpl_mesh with one sequence per clip.
    -> smpl_mesh's dict over [n_frames] rows and [n_clips] sequences."""
    pose_aa, trans, bad0 = smpl_of_bank(frames, clip_start, models, clip_model=clip_model, wait=bool(kw.get("wait", False)))
    dev = frames.device
    start = torch.as_tensor(clip_start).to(dev, torch.int64).contiguous()
    rows = torch.as_tensor(clip_len).to(dev, torch.int32).contiguous()
    b, g = _mesh_seq(betas, clip_gender, start.numel(), dev)
    res = smpl_mesh(mesh, pose_aa, trans, start, rows, b, seq_model=g, want=want, **kw)
    res["bad"] = res["bad"] + bad0
    return res
