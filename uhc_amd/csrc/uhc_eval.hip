// Evaluation on the device: uhc_eval_record, uhc_eval_record_pose, uhc_eval_metrics (include/uhc_amd.h).
//
// An evaluation episode (AgentCopycat.eval_seqs; reference: uhc/agents/agent_copycat.py:438-494) reads out, per control step and env, the humanoid's qpos, its
// joint positions and the expert frame it is compared with, and scores the trajectory at the end (uhc_amd/smpllib/smpl_eval.py).  Both halves are kernels here,
// so that the step loop needs no device -> host read: the caller owns the record arrays, the kernels append to them under per-env counters.
//
//   uhc_eval_record_kernel   one wave per env, four envs per workgroup.  Every lane reads the env's control words (alive, rows, done); the lanes copy the
//                            nqh + 72 doubles of the row; lane 0 writes the counters LAST (its stores depend on the words the whole wave loaded with it).
//   uhc_eval_record_pose_kernel  the same mapping: the 72 + 96 doubles (xpos / xquat of bodies 1 .. 24) of the row uhc_eval_record is about to append, for the
//                            contact quality (uhc_surface.hip).  It reads the row counter and leaves it to uhc_eval_record, which is enqueued behind it on the
//                            same stream; which env takes a snapshot, and into which row, is ev_snapshot_row for both.
//   uhc_eval_rows_kernel     one wave per TWO rows (lanes 0 .. 31 the even one, 32 .. 63 the odd one), four waves per workgroup; within a half lane = joint.
//                            The sums over the 24 joints are xor butterflies inside the half (16, 8, 4, 2, 1: every lane ends with the same bits, in an
//                            order fixed by the lane numbers alone); the 3 x 3 SVD of the Procrustes term is computed by every lane of the half alike.
//                            The arithmetic between the sums is uhc_eval_metrics.h, which the CPU test compiles for the host.
//   uhc_eval_means_kernel    one thread per (env, metric): the mean over the env's rows in row order.
// No floating-point atomics anywhere; the two counters that are added to (d_overflow, d_bad) are integers.  No row counter, whatever it holds, sends a read or
// a write outside the arrays (uhc_seq.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uhc_amd.h"
#include "uhc_api_check.h"
#include "uhc_device_env.h"

#pragma clang fp contract(off)
#include "uhc_eval_metrics.h"
#include "uhc_seq.h"

#define EV_NBODY 24
#define EV_NJ3 (3 * EV_NBODY)
#define EV_POSE_ROW (7 * EV_NBODY)  // a pose record's row: [24][3] positions, then [24][4] quaternions
#define EV_WAVES 4                  // waves per workgroup

// ------------------------------------------------------------------ the record
struct RecordArgs {
    int phase, n_env, nq, nqh, nbody, row_cap, t, fail_safe;
    const double *qpos, *xpos;  // [n_env][nq], [n_env][nbody][3] (body 0 = the world)
    const long long* clip0;     // [n_env] first bank frame of the env's clip
    const int* len;             // [n_env] frames of the env's clip
    const int* done;            // the step's outputs (phase 1)
    const double *reward, *percent_in;
    int *alive, *rows, *steps;
    double *pred_qpos, *pred_jpos;
    long long* gt_frame;
    double* rewards;
    int* fail_safe_out;
    double* percent;
    int *tele, *overflow;
};

// The snapshot rule of both record kernels, which must agree row for row: an env that is alive takes a snapshot before every step (phase 0), and once more (same
// t) after the step that ended its episode (phase 1, done).  -> the row of the env's record it goes to; EV_NO_ROOM when the counter is outside 0 .. row_cap - 1
// (nothing is written); EV_NO_SNAPSHOT when the env takes none.  done is read in phase 1 only, the counter only for a snapshot.
enum { EV_NO_SNAPSHOT = -1, EV_NO_ROOM = -2 };
__device__ __forceinline__ int ev_snapshot_row(int phase, const int* alive, const int* done, const int* rows, int row_cap, int e) {
    if (alive[e] == 0) return EV_NO_SNAPSHOT;
    if (!(phase == 0 || done[e] != 0)) return EV_NO_SNAPSHOT;
    const int r = rows[e];
    return r < 0 || r >= row_cap ? EV_NO_ROOM : r;
}

__global__ void __launch_bounds__(64 * EV_WAVES) uhc_eval_record_kernel(const RecordArgs A) {
    const int lane = threadIdx.x & 63, e = blockIdx.x * EV_WAVES + (threadIdx.x >> 6);
    if (e >= A.n_env) return;
    const bool alive = A.alive[e] != 0;
    if (!alive) {
        if (A.phase == 1 && lane == 0) A.tele[e] = 0;
        return;
    }
    const bool done = A.phase == 1 && A.done[e] != 0;
    const int rows = ev_snapshot_row(A.phase, A.alive, A.done, A.rows, A.row_cap, e);
    if (rows != EV_NO_SNAPSHOT) {
        if (rows == EV_NO_ROOM) {
            if (lane == 0) atomicAdd(A.overflow, 1);  // (an integer count; nothing is written)
        } else {
            const size_t row = (size_t)e * A.row_cap + rows;
            const double* q = A.qpos + (size_t)e * A.nq;
            const double* x = A.xpos + (size_t)e * A.nbody * 3 + 3;  // bodies 1 .. 24
            for (int j = lane; j < A.nqh; j += 64) A.pred_qpos[row * A.nqh + j] = q[j];
            for (int j = lane; j < EV_NJ3; j += 64) A.pred_jpos[row * EV_NJ3 + j] = x[j];
            if (lane == 0) {
                const int last = A.len[e] - 1;
                A.gt_frame[row] = A.clip0[e] + (long long)(A.t < last ? A.t : last);
                A.rows[e] = rows + 1;
            }
        }
    }
    if (A.phase == 1 && lane == 0) {
        const int steps = A.steps[e];
        if (steps >= 0 && steps < A.row_cap) {
            A.rewards[(size_t)e * A.row_cap + steps] = A.reward[e];
            A.steps[e] = steps + 1;
        }
        int tele = 0;
        if (done) {
            const double pct = A.percent_in[e];
            if (A.fail_safe && pct != 1.0) {  // the caller teleports the env to the expert pose and the episode goes on (humanoid_im.py:902-905)
                A.fail_safe_out[e] = 1;
                tele = 1;
            } else {
                A.alive[e] = 0;
                A.percent[e] = pct;
            }
        }
        A.tele[e] = tele;
    }
}

// ------------------------------------------------------------------ the pose record
struct RecordPoseArgs {
    int phase, n_env, nbody, row_cap;
    const double *xpos, *xquat;  // [n_env][nbody][3], [n_env][nbody][4] (body 0 = the world)
    const int *done, *alive, *rows;
    double* pose;  // [n_env][row_cap][168]
};

__global__ void __launch_bounds__(64 * EV_WAVES) uhc_eval_record_pose_kernel(const RecordPoseArgs A) {
    const int lane = threadIdx.x & 63, e = blockIdx.x * EV_WAVES + (threadIdx.x >> 6);
    if (e >= A.n_env) return;
    const int rows = ev_snapshot_row(A.phase, A.alive, A.done, A.rows, A.row_cap, e);
    if (rows < 0) return;  // (no snapshot, or no room: uhc_eval_record counts the overflow)
    double* out = A.pose + ((size_t)e * A.row_cap + rows) * EV_POSE_ROW;
    const double* x = A.xpos + (size_t)e * A.nbody * 3 + 3;  // bodies 1 .. 24
    const double* q = A.xquat + (size_t)e * A.nbody * 4 + 4;
    for (int j = lane; j < 3 * EV_NBODY; j += 64) out[j] = x[j];
    for (int j = lane; j < 4 * EV_NBODY; j += 64) out[3 * EV_NBODY + j] = q[j];
}

// ------------------------------------------------------------------ the metrics
struct MetricArgs {
    int n_env, nqh, row_cap;
    long long n_frames;
    const int* rows;
    const double *pred_qpos, *pred_jpos;
    const long long* gt_frame;
    const double* frames;
    double *row_metrics, *clip_means;
    int* bad;
};

__global__ void __launch_bounds__(64 * EV_WAVES) uhc_eval_rows_kernel(const MetricArgs A) {
    const int lane = threadIdx.x & 63, joint = lane & 31;
    const long long R = ((long long)blockIdx.x * EV_WAVES + (threadIdx.x >> 6)) * 2 + (lane >> 5);
    const long long n_rows_all = (long long)A.n_env * A.row_cap;
    // (no lane leaves before the last butterfly: a half without a row computes on zeros and stores nothing)
    const bool in_grid = R < n_rows_all;
    const int e = in_grid ? (int)(R / A.row_cap) : 0, r = in_grid ? (int)(R % A.row_cap) : 0;
    const int T = uhc_seq_rows(A.rows[e], A.row_cap);
    const bool valid = in_grid && r < T;
    const int n_next = !valid ? 0 : (T - 1 - r < 2 ? T - 1 - r : 2);
    const bool has_joint = joint < EV_NBODY;
    const int j = has_joint ? joint : 0;

    // the gt frames of rows r, r + 1, r + 2: an index outside the bank is not followed
    long long f[3] = {0, 0, 0};
    bool ok[3] = {false, false, false};
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (valid && k <= n_next) {
            f[k] = A.gt_frame[(size_t)e * A.row_cap + r + k];
            ok[k] = f[k] >= 0 && f[k] < A.n_frames;
        }
    if (valid && !ok[0] && joint == 0) atomicAdd(A.bad, 1);  // one count per bad entry: by the row that owns it
    UhcEmV3 p[3], g[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        p[k] = g[k] = {0.0, 0.0, 0.0};
        if (valid && k <= n_next && has_joint) {
            const double* pp = A.pred_jpos + ((size_t)e * A.row_cap + r + k) * EV_NJ3 + 3 * j;
            p[k] = {pp[0], pp[1], pp[2]};
            if (ok[k]) {
                const double* gp = A.frames + (size_t)f[k] * UHC_FRAME_STRIDE + UHC_FR_WBPOS + 3 * j;
                g[k] = {gp[0], gp[1], gp[2]};
            }
        }
    }
    const int root_lane = lane & 32;  // joint 0 of the half
    const UhcEmV3 pr = {__shfl(p[0].x, root_lane), __shfl(p[0].y, root_lane), __shfl(p[0].z, root_lane)};
    const UhcEmV3 gr = {__shfl(g[0].x, root_lane), __shfl(g[0].y, root_lane), __shfl(g[0].z, root_lane)};
    UhcEmJoint J = uhc_em_joint_norms(p, g, pr, gr);
    if (!has_joint) J.g = J.m = J.vel = J.acc = 0.0, J.p0 = J.g0 = {0.0, 0.0, 0.0};
    const double sg = uhc_xor_sum<16>(J.g), sm = uhc_xor_sum<16>(J.m), sv = uhc_xor_sum<16>(J.vel), sa = uhc_xor_sum<16>(J.acc);
    const UhcEmV3 muX = {uhc_xor_sum<16>(J.g0.x) / EV_NBODY, uhc_xor_sum<16>(J.g0.y) / EV_NBODY, uhc_xor_sum<16>(J.g0.z) / EV_NBODY};
    const UhcEmV3 muY = {uhc_xor_sum<16>(J.p0.x) / EV_NBODY, uhc_xor_sum<16>(J.p0.y) / EV_NBODY, uhc_xor_sum<16>(J.p0.z) / EV_NBODY};
    UhcEmV3 x0 = {J.g0.x - muX.x, J.g0.y - muX.y, J.g0.z - muX.z}, y0 = {J.p0.x - muY.x, J.p0.y - muY.y, J.p0.z - muY.z};
    if (!has_joint) x0 = y0 = {0.0, 0.0, 0.0};
    const double nX = sqrt(uhc_xor_sum<16>(x0.x * x0.x + x0.y * x0.y + x0.z * x0.z)), nY = sqrt(uhc_xor_sum<16>(y0.x * y0.x + y0.y * y0.y + y0.z * y0.z));
    const double xn[3] = {x0.x / nX, x0.y / nX, x0.z / nX}, yn[3] = {y0.x / nY, y0.y / nY, y0.z / nY};
    double H[9];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) H[3 * a + b] = uhc_xor_sum<16>(has_joint ? xn[a] * yn[b] : 0.0);
    const UhcEmAlign Al = uhc_em_procrustes(H, nX, nY, muX, muY);
    const double sp = uhc_xor_sum<16>(has_joint ? uhc_em_aligned_err(Al, J.p0, J.g0) : 0.0);

    if (valid && joint == 0) {
        const double nan = uhc_nan();
        double* out = A.row_metrics + ((size_t)e * A.row_cap + r) * UHC_EM_NMETRIC;
        double root = nan;
        if (ok[0]) root = uhc_em_root_err(A.pred_qpos + ((size_t)e * A.row_cap + r) * A.nqh, A.frames + (size_t)f[0] * UHC_FRAME_STRIDE + UHC_FR_QPOS) / T * 1000.0;
        out[UHC_EM_ROOT_DIST] = root;
        if (n_next >= 1) out[UHC_EM_VEL_DIST] = ok[0] && ok[1] ? sv / EV_NBODY * 1000.0 : nan;
        if (n_next >= 2) out[UHC_EM_ACCEL_DIST] = ok[0] && ok[1] && ok[2] ? sa / EV_NBODY * 1000.0 : nan;
        out[UHC_EM_MPJPE_G] = ok[0] ? sg / EV_NBODY * 1000.0 : nan;
        out[UHC_EM_PA_MPJPE] = ok[0] ? sp / EV_NBODY * 1000.0 : nan;
        out[UHC_EM_MPJPE] = ok[0] ? sm / EV_NBODY * 1000.0 : nan;
    }
}

__global__ void __launch_bounds__(256) uhc_eval_means_kernel(const MetricArgs A) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= A.n_env * UHC_EM_NMETRIC) return;
    const int e = idx / UHC_EM_NMETRIC, k = idx % UHC_EM_NMETRIC;
    const int T = uhc_seq_rows(A.rows[e], A.row_cap);
    const int n = T - (k == UHC_EM_VEL_DIST ? 1 : (k == UHC_EM_ACCEL_DIST ? 2 : 0));  // numpy's lengths: T, T - 1 for the velocity, T - 2 for the acceleration
    A.clip_means[idx] = uhc_seq_mean(A.row_metrics, UHC_EM_NMETRIC, k, (long long)e * A.row_cap, n);
}

// ------------------------------------------------------------------ C-ABI (include/uhc_amd.h)
extern "C" int32_t uhc_eval_record(void* stream, int32_t phase, int32_t n_env, int32_t n_body, int32_t nq, int32_t nqh, int32_t nbody, int32_t row_cap,
                                   int32_t t, int32_t fail_safe, const double* d_qpos, const double* d_xpos, const int64_t* d_clip0, const int32_t* d_len,
                                   const int32_t* d_done, const double* d_reward, const double* d_percent_in, int32_t* d_alive, int32_t* d_rows,
                                   int32_t* d_steps, double* d_pred_qpos, double* d_pred_jpos, int64_t* d_gt_frame, double* d_rewards,
                                   int32_t* d_fail_safe, double* d_percent, int32_t* d_tele, int32_t* d_overflow) {
    // every check comes before the first HIP call
    REFUSE("uhc_eval_record", phase != 0 && phase != 1, "phase must be 0 (before the step) or 1 (after it)");
    REFUSE("uhc_eval_record", n_env < 0, "n_env < 0");
    REFUSE("uhc_eval_record", n_body != EV_NBODY, "n_body must be 24 (a row holds 72 joint coordinates)");
    REFUSE("uhc_eval_record", nqh < 7 || nqh > nq, "nqh must be 7 .. nq");
    REFUSE("uhc_eval_record", nbody < n_body + 1, "nbody must be at least n_body + 1 (the world body comes first)");
    REFUSE("uhc_eval_record", row_cap <= 0, "row_cap <= 0");
    REFUSE("uhc_eval_record", t < 0, "t < 0");
    REFUSE("uhc_eval_record", !d_qpos, "d_qpos is NULL");
    REFUSE("uhc_eval_record", !d_xpos, "d_xpos is NULL");
    REFUSE("uhc_eval_record", !d_clip0, "d_clip0 is NULL");
    REFUSE("uhc_eval_record", !d_len, "d_len is NULL");
    REFUSE("uhc_eval_record", phase == 1 && !d_done, "d_done is NULL");
    REFUSE("uhc_eval_record", phase == 1 && !d_reward, "d_reward is NULL");
    REFUSE("uhc_eval_record", phase == 1 && !d_percent_in, "d_percent_in is NULL");
    REFUSE("uhc_eval_record", !d_alive, "d_alive is NULL");
    REFUSE("uhc_eval_record", !d_rows, "d_rows is NULL");
    REFUSE("uhc_eval_record", !d_steps, "d_steps is NULL");
    REFUSE("uhc_eval_record", !d_pred_qpos, "d_pred_qpos is NULL");
    REFUSE("uhc_eval_record", !d_pred_jpos, "d_pred_jpos is NULL");
    REFUSE("uhc_eval_record", !d_gt_frame, "d_gt_frame is NULL");
    REFUSE("uhc_eval_record", !d_rewards, "d_rewards is NULL");
    REFUSE("uhc_eval_record", !d_fail_safe, "d_fail_safe is NULL");
    REFUSE("uhc_eval_record", !d_percent, "d_percent is NULL");
    REFUSE("uhc_eval_record", !d_tele, "d_tele is NULL");
    REFUSE("uhc_eval_record", !d_overflow, "d_overflow is NULL");
    if (n_env == 0) return 0;
    RecordArgs A = {};
    A.phase = phase, A.n_env = n_env, A.nq = nq, A.nqh = nqh, A.nbody = nbody, A.row_cap = row_cap, A.t = t, A.fail_safe = fail_safe != 0;
    A.qpos = d_qpos, A.xpos = d_xpos, A.clip0 = (const long long*)d_clip0, A.len = d_len, A.done = d_done, A.reward = d_reward, A.percent_in = d_percent_in;
    A.alive = d_alive, A.rows = d_rows, A.steps = d_steps, A.pred_qpos = d_pred_qpos, A.pred_jpos = d_pred_jpos, A.gt_frame = (long long*)d_gt_frame;
    A.rewards = d_rewards, A.fail_safe_out = d_fail_safe, A.percent = d_percent, A.tele = d_tele, A.overflow = d_overflow;
    hipLaunchKernelGGL(uhc_eval_record_kernel, dim3((unsigned)((n_env + EV_WAVES - 1) / EV_WAVES)), dim3(64 * EV_WAVES), 0, (hipStream_t)stream, A);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int32_t uhc_eval_record_pose(void* stream, int32_t phase, int32_t n_env, int32_t nbody, int32_t row_cap, const double* d_xpos, const double* d_xquat,
                                        const int32_t* d_done, const int32_t* d_alive, const int32_t* d_rows, double* d_pose) {
    REFUSE("uhc_eval_record_pose", phase != 0 && phase != 1, "phase must be 0 (before the step) or 1 (after it)");
    REFUSE("uhc_eval_record_pose", n_env < 0, "n_env < 0");
    REFUSE("uhc_eval_record_pose", nbody < EV_NBODY + 1, "nbody must be at least 25 (the world body comes first, a row holds 24 poses)");
    REFUSE("uhc_eval_record_pose", row_cap <= 0, "row_cap <= 0");
    REFUSE("uhc_eval_record_pose", !d_xpos, "d_xpos is NULL");
    REFUSE("uhc_eval_record_pose", !d_xquat, "d_xquat is NULL");
    REFUSE("uhc_eval_record_pose", phase == 1 && !d_done, "d_done is NULL");
    REFUSE("uhc_eval_record_pose", !d_alive, "d_alive is NULL");
    REFUSE("uhc_eval_record_pose", !d_rows, "d_rows is NULL");
    REFUSE("uhc_eval_record_pose", !d_pose, "d_pose is NULL");
    if (n_env == 0) return 0;
    RecordPoseArgs A = {};
    A.phase = phase, A.n_env = n_env, A.nbody = nbody, A.row_cap = row_cap, A.xpos = d_xpos, A.xquat = d_xquat, A.done = d_done, A.alive = d_alive, A.rows = d_rows;
    A.pose = d_pose;
    hipLaunchKernelGGL(uhc_eval_record_pose_kernel, dim3((unsigned)((n_env + EV_WAVES - 1) / EV_WAVES)), dim3(64 * EV_WAVES), 0, (hipStream_t)stream, A);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int32_t uhc_eval_metrics(void* stream, int32_t n_env, int32_t n_body, int32_t nqh, int32_t row_cap, const int32_t* d_rows,
                                    const double* d_pred_qpos, const double* d_pred_jpos, const int64_t* d_gt_frame, const double* d_frames,
                                    int64_t n_frames, double* d_row_metrics, double* d_clip_means, int32_t* d_bad, int32_t* h_bad) {
    REFUSE("uhc_eval_metrics", n_env < 0, "n_env < 0");
    REFUSE("uhc_eval_metrics", n_body != EV_NBODY, "n_body must be 24 (UHC_FRAME_STRIDE is a 24-body layout)");
    REFUSE("uhc_eval_metrics", nqh < 7, "nqh must be at least 7");
    REFUSE("uhc_eval_metrics", row_cap <= 0, "row_cap <= 0");
    REFUSE("uhc_eval_metrics", n_frames < 0, "n_frames < 0");
    REFUSE("uhc_eval_metrics", !d_rows, "d_rows is NULL");
    REFUSE("uhc_eval_metrics", !d_pred_qpos, "d_pred_qpos is NULL");
    REFUSE("uhc_eval_metrics", !d_pred_jpos, "d_pred_jpos is NULL");
    REFUSE("uhc_eval_metrics", !d_gt_frame, "d_gt_frame is NULL");
    REFUSE("uhc_eval_metrics", !d_frames, "d_frames is NULL");
    REFUSE("uhc_eval_metrics", !d_row_metrics, "d_row_metrics is NULL");
    REFUSE("uhc_eval_metrics", !d_clip_means, "d_clip_means is NULL");
    REFUSE("uhc_eval_metrics", !d_bad, "d_bad is NULL");
    const long long blocks = ((long long)n_env * row_cap + 2 * EV_WAVES - 1) / (2 * EV_WAVES);
    REFUSE("uhc_eval_metrics", !uhc_launch_fits(blocks) || !uhc_launch_fits((long long)n_env * UHC_EM_NMETRIC), "n_env x row_cap is beyond one launch");
    if (n_env == 0) {
        if (h_bad) *h_bad = 0;
        return 0;
    }
    MetricArgs A = {};
    A.n_env = n_env, A.nqh = nqh, A.row_cap = row_cap, A.n_frames = n_frames, A.rows = d_rows, A.pred_qpos = d_pred_qpos, A.pred_jpos = d_pred_jpos;
    A.gt_frame = (const long long*)d_gt_frame, A.frames = d_frames, A.row_metrics = d_row_metrics, A.clip_means = d_clip_means, A.bad = d_bad;
    hipStream_t s = (hipStream_t)stream;
    HIP_OK(hipMemsetAsync(d_bad, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(uhc_eval_rows_kernel, dim3((unsigned)blocks), dim3(64 * EV_WAVES), 0, s, A);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(uhc_eval_means_kernel, dim3((unsigned)((n_env * UHC_EM_NMETRIC + 255) / 256)), dim3(256), 0, s, A);
    HIP_OK(hipGetLastError());
    return uhc_return_bad(h_bad, d_bad, s);
}
