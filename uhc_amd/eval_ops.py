"""Host side of the evaluation kernels (uhc_amd/csrc/uhc_eval.hip; C-ABI in include/uhc_amd.h): thin ctypes calls on torch tensors, like rollout_ops.
The record of an episode batch -- what eval_seqs reads out per control step -- lives in torch tensors the caller owns (Record); uhc_eval_record appends
to it on the device, uhc_eval_metrics scores it against the clip bank.  Device float64 / int32 / int64 only; there is no CPU path."""
import ctypes as C

import torch

from ._lib import check, lib

N_BODY = 24
METRICS = ("root_dist", "vel_dist", "accel_dist", "mpjpe_g", "pa_mpjpe", "mpjpe")  # the order of a row of row_metrics (uhc_eval_metrics.h)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class Record:
    """The caller-owned state of uhc_eval_record for n_env envs, zeroed: up to row_cap rows per env."""

    def __init__(self, n_env, row_cap, nqh, device):
        z = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device=device)
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
