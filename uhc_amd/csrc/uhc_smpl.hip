// AMASS axis-angle poses -> qpos rows, computed on the device: uhc_smpl_qpos (include/uhc_amd.h); the same from 6D rows: uhc_smpl6d_qpos; and the way back,
// qpos rows -> axis-angle poses, translation and 6D rows: uhc_qpos_smpl (further down).
//
// The step in front of uhc_expert_frames: smpl_to_qpose (uhc_amd/smpllib/smpl_mujoco.py; reference: uhc/smpllib/smpl_mujoco.py:543-607) is a pure map over
// (frame, joint) -- rotation vector -> quaternion -> intrinsic ZYX Euler angles (the hinge humanoid) or the quaternion itself (the ball-joint humanoid) --,
// reordered from SMPL joint order to the model's depth-first body order.  A frame reads 576 B of pose and 24 B of translation and writes 608 B and / or 792 B.
//
// Mapping: one lane per (frame, SMPL joint), 24 lanes a frame, SC_FRAMES frames a workgroup (a frame's lanes may sit in two waves: no lane talks to another).
//   lane (f, j)     reads joint j's 24 bytes -- a workgroup's lanes read one run of consecutive addresses --, forms the quaternion and from it the hinge triple
//                   and / or the (w, x, y, z) quadruple in registers, and puts them into slot slot_of_joint[j] of the frame's row(s) in LDS.
//   lane (f, 0)     also forms the root quaternion of the 76-wide row (through the rotation matrix: the branch rule that fixes its sign) and the root position:
//                   trans + root_offset[model of the frame's clip]; the clip is the lane's own binary search in d_clip_start (uhc_seq.h: uhc_clip_of).
//   all lanes       copy the workgroup's rows out, 16 B per lane to consecutive addresses.  A workgroup starts at an even frame, so its rows start 16-byte
//                   aligned (8 x 608 B, 8 x 792 B); an odd number of 99-wide rows (the bank's tail) ends in one 8-byte store.
// No array is indexed at run time by a value read from memory: the slot table arrives packed in kernel-argument words (checked on the host to be a
// permutation), a clip's model index is range-checked before it selects a root offset (uhc_seq.h).  No atomics; no scratch.
//
// Arithmetic: uhc_smpl_convert.h, scipy's formulas one for one, products and sums rounded separately (no FMA contraction), so that what differs from the
// host path are the last bits of sqrt / sin / cos / atan2 / hypot alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uhc_amd.h"
#include "uhc_api_check.h"
#include "uhc_seq.h"
#include "uhc_smpl_convert.h"

#pragma clang fp contract(off)

#define SC_FRAMES 8                        // frames per workgroup (even: see above)
#define SC_THREADS (SC_FRAMES * UHC_SC_NJ)  // 192: three waves

struct SmplArgs {
    const double* pose;         // [n_frames][72]
    const double* trans;        // [n_frames][3] or NULL
    const double* root_offset;  // [n_models][3] or NULL
    const int* clip_start;      // [n_clips]
    const int* clip_model;      // [n_clips] or NULL
    double* qpos;               // [n_frames][76] or NULL
    double* qpos_quat;          // [n_frames][99] or NULL
    long long n_frames;
    int n_clips, n_models;
    unsigned long long slot[3];  // the model slot of SMPL joint j, one byte per joint
};

// The body of both kernels that write qpos rows.  SIX = false: A.pose holds rotation vectors [n_frames][72] and A.trans the translations (uhc_smpl_qpos);
// SIX = true: A.pose holds 6D rows [n_frames][147] = translation | 24 x (column 0, column 1), the joint's quaternion comes from uhc_sc_rot6d_quat and the
// translation from the row's head (uhc_smpl6d_qpos).  Behind the quaternion the two are the same code.
template <bool SIX>
__device__ __forceinline__ void smpl_qpos_rows(const SmplArgs& A, double* row_s, double* quat_s) {
    const int tid = threadIdx.x, fl = tid / UHC_SC_NJ, j = tid - fl * UHC_SC_NJ;
    const long long f0 = (long long)blockIdx.x * SC_FRAMES, f = f0 + fl;
    if (f < A.n_frames) {
        UhcScQuat q;
        if (SIX) {
            const double* r = A.pose + (size_t)f * UHC_SC_N6D + 3 + 6 * j;
            q = uhc_sc_rot6d_quat({r[0], r[1], r[2], r[3], r[4], r[5]});
        } else {
            const double* r = A.pose + (size_t)f * (3 * UHC_SC_NJ) + 3 * j;
            q = uhc_sc_rotvec_quat(r[0], r[1], r[2]);
        }
        const int m = uhc_packed_byte(A.slot, j);  // (a permutation of 0 .. 23 with slot[0] = 0: checked before the launch)
        double* row = row_s + fl * UHC_SC_NQ;
        double* qrow = quat_s + fl * UHC_SC_NQ_QUAT;
        if (A.qpos_quat) {
            double* o = qrow + 3 + 4 * m;
            o[0] = q.w, o[1] = q.x, o[2] = q.y, o[3] = q.z;
        }
        if (j == 0) {
            // ---- the frame's clip: all it decides is which model's root offset the row gets
            const double* off = nullptr;
            if (A.root_offset) off = A.root_offset + (size_t)uhc_seq_model(A.clip_model, uhc_clip_of(A.clip_start, A.n_clips, f), A.n_models) * 3;
            const UhcScV3 p = uhc_sc_root_pos(SIX ? A.pose + (size_t)f * UHC_SC_N6D : (A.trans ? A.trans + (size_t)f * 3 : nullptr), off);
            if (A.qpos) {
                double R[9];
                uhc_sc_quat_matrix(q, R);
                const UhcScQ4 rq = uhc_sc_root_quat(R);
                row[0] = p.x, row[1] = p.y, row[2] = p.z;
                row[3] = rq.w, row[4] = rq.x, row[5] = rq.y, row[6] = rq.z;
            }
            if (A.qpos_quat) qrow[0] = p.x, qrow[1] = p.y, qrow[2] = p.z;
        } else if (A.qpos) {
            const UhcScEuler e = uhc_sc_quat_euler_zyx(q);
            double* o = row + 7 + 3 * (m - 1);
            o[0] = e.Z, o[1] = e.Y, o[2] = e.X;
        }
    }
    __syncthreads();
    const long long left = A.n_frames - f0;
    const int nf = left < SC_FRAMES ? (int)left : SC_FRAMES;  // (>= 1: the grid has no empty workgroup)
    if (A.qpos) {
        const double2* src = reinterpret_cast<const double2*>(row_s);
        double2* dst = reinterpret_cast<double2*>(A.qpos + (size_t)f0 * UHC_SC_NQ);  // 608 B a row: 16-byte aligned at every frame
        for (int k = tid; k < nf * (UHC_SC_NQ / 2); k += SC_THREADS) dst[k] = src[k];
    }
    if (A.qpos_quat) {
        const int n = nf * UHC_SC_NQ_QUAT;
        const double2* src = reinterpret_cast<const double2*>(quat_s);
        double* out = A.qpos_quat + (size_t)f0 * UHC_SC_NQ_QUAT;  // 792 B a row: 16-byte aligned at every EVEN frame, and f0 is one
        double2* dst = reinterpret_cast<double2*>(out);
        for (int k = tid; k < n / 2; k += SC_THREADS) dst[k] = src[k];
        if ((n & 1) && tid == 0) out[n - 1] = quat_s[n - 1];
    }
}

__global__ void __launch_bounds__(SC_THREADS) uhc_smpl_qpos_kernel(const SmplArgs A) {
    __shared__ __attribute__((aligned(16))) double row_s[SC_FRAMES * UHC_SC_NQ];        // the workgroup's 76-wide rows, one behind the other as in d_qpos
    __shared__ __attribute__((aligned(16))) double quat_s[SC_FRAMES * UHC_SC_NQ_QUAT];  // ... and its 99-wide rows
    smpl_qpos_rows<false>(A, row_s, quat_s);
}

__global__ void __launch_bounds__(SC_THREADS) uhc_smpl6d_qpos_kernel(const SmplArgs A) {
    __shared__ __attribute__((aligned(16))) double row_s[SC_FRAMES * UHC_SC_NQ];
    __shared__ __attribute__((aligned(16))) double quat_s[SC_FRAMES * UHC_SC_NQ_QUAT];
    smpl_qpos_rows<true>(A, row_s, quat_s);
}

// ------------------------------------------------------------------ the way back: qpos rows -> pose_aa / trans / full_6d (uhc_qpos_smpl)
// Same mapping: one lane per (row, SMPL joint), 24 lanes a row, SC_FRAMES rows a workgroup.  Global row g = s * row_cap + r is row r of sequence s and lies at
// d_qpos + g * stride; with d_seq_rows only r < clamp(seq_rows[s], 0, row_cap) is converted and every other output slot keeps what it held.
//   lanes 0 .. 7    decide whether the workgroup's rows are live (the one read of d_seq_rows) and clear their bad flags
//   all lanes       stage the live rows through LDS, consecutive lanes reading consecutive addresses of a row: 16 bytes a lane where stride and base are
//                   both even (decided on the host: vec_in), else 8 -- a stride of 83 doubles keeps rows 8-byte aligned only
//   lane (row, j)   forms joint j's unit quaternion from slot slot_of_joint[j] of the staged row (hinge triple -> from_euler; root and ball joints ->
//                   from_quat's normalisation), from it the rotation vector and / or the two matrix columns, into the row's output rows in LDS; a quaternion of
//                   zero or non-finite norm raises the row's bad flag (a plain LDS store of 1: every writer writes the same value)
//   lane (row, 0)   also forms trans = qpos[:3] - root_offset[model of the sequence] (the model index range-checked), and, for a bad row, adds 1 to d_bad: the
//                   kernel's one atomic, a vector atomic add, once per bad row
//   all lanes       copy the live rows out, 16 B per lane; a workgroup starts at a multiple of 8 rows, so its first output row is 16-byte aligned at every
//                   width (576, 24 and 1176 B a row); a pair that straddles a dead row or the end goes out as one 8-byte store.  A bad row goes out as NaN.
// No array is indexed at run time by a value read from memory other than the range-checked model index; no scratch.
struct PoseArgs {
    const double* qpos;         // row g at qpos + g * stride
    const double* root_offset;  // [n_models][3] or NULL
    const int* seq_rows;        // [n_seq] or NULL
    const int* seq_model;       // [n_seq] or NULL
    double* pose_aa;            // [n_rows][72] or NULL
    double* trans;              // [n_rows][3] or NULL
    double* full_6d;            // [n_rows][147] or NULL
    int* bad;                   // [1]
    long long stride, n_rows;   // n_rows = n_seq * row_cap
    int row_cap, n_models, ball, vec_in;
    unsigned long long slot[3];
};

#define SP_PITCH 100  // a staged row in LDS: 76 or 99 doubles, even pitch so that every row starts 16-byte aligned

// the workgroup's live rows out of LDS (W doubles a row, one behind the other) to out (the workgroup's first row; 16-byte aligned), NaN for a bad row
template <int W>
__device__ __forceinline__ void pose_rows_out(double* out, const double* lds, const int* live_s, const int* bad_s, int nf, int tid) {
    const double nan = uhc_nan();
    const int n = nf * W;
    for (int k = tid; 2 * k < n; k += SC_THREADS) {
        const int i0 = 2 * k, i1 = i0 + 1, r0 = i0 / W, r1 = i1 < n ? i1 / W : r0;
        const bool l0 = live_s[r0] != 0, l1 = i1 < n && live_s[r1] != 0;
        const double2 v = *reinterpret_cast<const double2*>(lds + i0);  // (i1 == n, W odd: the double behind the last row, inside the array and not used)
        const double v0 = bad_s[r0] ? nan : v.x, v1 = bad_s[r1] ? nan : v.y;
        if (l0 && l1) *reinterpret_cast<double2*>(out + i0) = make_double2(v0, v1);
        else if (l0) out[i0] = v0;
        else if (l1) out[i1] = v1;
    }
}

__global__ void __launch_bounds__(SC_THREADS) uhc_qpos_smpl_kernel(const PoseArgs A) {
    __shared__ __attribute__((aligned(16))) double in_s[SC_FRAMES * SP_PITCH];
    __shared__ __attribute__((aligned(16))) double pose_s[SC_FRAMES * 3 * UHC_SC_NJ];
    __shared__ __attribute__((aligned(16))) double trans_s[SC_FRAMES * 3];
    __shared__ __attribute__((aligned(16))) double six_s[SC_FRAMES * UHC_SC_N6D];
    __shared__ int live_s[SC_FRAMES], bad_s[SC_FRAMES];
    const int tid = threadIdx.x, fl = tid / UHC_SC_NJ, j = tid - fl * UHC_SC_NJ;
    const long long g0 = (long long)blockIdx.x * SC_FRAMES;
    const long long left = A.n_rows - g0;
    const int nf = left < SC_FRAMES ? (int)left : SC_FRAMES;  // (>= 1: the grid has no empty workgroup)
    const int width = A.ball ? UHC_SC_NQ_QUAT : UHC_SC_NQ;
    if (tid < SC_FRAMES) {
        int live = 0;
        if (tid < nf) {
            live = 1;
            if (A.seq_rows) {
                const long long g = g0 + tid, s = g / A.row_cap;
                live = (int)(g - s * A.row_cap) < uhc_seq_rows(A.seq_rows[s], A.row_cap);
            }
        }
        live_s[tid] = live, bad_s[tid] = 0;
    }
    __syncthreads();
    // ---- stage: row rr of the workgroup, consecutive lanes on consecutive addresses
    if (A.vec_in) {
        const int w2 = width >> 1;  // 38, or 49 and one double behind
        for (int k = tid; k < SC_FRAMES * w2; k += SC_THREADS) {
            const int rr = k / w2, c = k - rr * w2;
            if (live_s[rr]) *reinterpret_cast<double2*>(in_s + rr * SP_PITCH + 2 * c) = *reinterpret_cast<const double2*>(A.qpos + (size_t)(g0 + rr) * A.stride + 2 * c);
        }
        if ((width & 1) && tid < SC_FRAMES && live_s[tid]) in_s[tid * SP_PITCH + width - 1] = A.qpos[(size_t)(g0 + tid) * A.stride + width - 1];
    } else {
        for (int k = tid; k < SC_FRAMES * width; k += SC_THREADS) {
            const int rr = k / width, c = k - rr * width;
            if (live_s[rr]) in_s[rr * SP_PITCH + c] = A.qpos[(size_t)(g0 + rr) * A.stride + c];
        }
    }
    __syncthreads();
    if (live_s[fl]) {
        const double* row = in_s + fl * SP_PITCH;
        UhcScQuat q;
        const bool ok = uhc_sc_row_joint_quat(row, A.ball, j, uhc_packed_byte(A.slot, j), q);  // (the slot: a permutation of 0 .. 23 with slot[0] = 0, checked before the launch)
        if (!ok) bad_s[fl] = 1;
        if (A.pose_aa) {
            const UhcScV3 r = uhc_sc_quat_rotvec(q);
            double* o = pose_s + fl * (3 * UHC_SC_NJ) + 3 * j;
            o[0] = r.x, o[1] = r.y, o[2] = r.z;
        }
        if (A.full_6d) {
            const UhcScRot6 s = uhc_sc_quat_rot6d(q);
            double* o = six_s + fl * UHC_SC_N6D + 3 + 6 * j;
            o[0] = s.ax, o[1] = s.ay, o[2] = s.az, o[3] = s.bx, o[4] = s.by, o[5] = s.bz;
        }
        if (j == 0) {
            double ox = 0.0, oy = 0.0, oz = 0.0;
            if (A.root_offset) {
                const double* off = A.root_offset + (size_t)uhc_seq_model(A.seq_model, (g0 + fl) / A.row_cap, A.n_models) * 3;
                ox = off[0], oy = off[1], oz = off[2];
            }
            const double tx = row[0] - ox, ty = row[1] - oy, tz = row[2] - oz;
            if (A.trans) trans_s[3 * fl] = tx, trans_s[3 * fl + 1] = ty, trans_s[3 * fl + 2] = tz;
            if (A.full_6d) {
                double* o = six_s + fl * UHC_SC_N6D;
                o[0] = tx, o[1] = ty, o[2] = tz;
            }
        }
    }
    __syncthreads();
    if (tid < SC_FRAMES && live_s[tid] && bad_s[tid]) atomicAdd(A.bad, 1);
    if (A.pose_aa) pose_rows_out<3 * UHC_SC_NJ>(A.pose_aa + (size_t)g0 * (3 * UHC_SC_NJ), pose_s, live_s, bad_s, nf, tid);
    if (A.trans) pose_rows_out<3>(A.trans + (size_t)g0 * 3, trans_s, live_s, bad_s, nf, tid);
    if (A.full_6d) pose_rows_out<UHC_SC_N6D>(A.full_6d + (size_t)g0 * UHC_SC_N6D, six_s, live_s, bad_s, nf, tid);
}

// ------------------------------------------------------------------ C-ABI (include/uhc_amd.h)
// h_smpl_to_model [24] -> the model slot of every SMPL joint, one byte a joint; refused unless it is a permutation of 0 .. 23 that keeps the root at 0
static int pack_slot_table(const char* fn, const int32_t* h_smpl_to_model, unsigned long long (&slot)[3]) {
    unsigned seen = 0;
    for (int m = 0; m < UHC_SC_NJ; m++) {
        const int j = h_smpl_to_model[m];
        if (j < 0 || j >= UHC_SC_NJ || (seen >> j & 1u) || (m == 0) != (j == 0))
            return uhc_internal_set_error((std::string(fn) + ": h_smpl_to_model[" + std::to_string(m) + "] = " + std::to_string(j) +
                                           ": the table is a permutation of 0 .. 23 that keeps the root at 0").c_str());
        seen |= 1u << j;
        slot[j >> 3] |= (unsigned long long)m << (8 * (j & 7));
    }
    return 0;
}

// uhc_smpl_qpos (d_pose_aa, d_trans) and uhc_smpl6d_qpos (d_full_6d): one set of checks, one launch
static int smpl_qpos_launch(const char* fn, bool six, void* stream, int32_t n_joint, const int32_t* h_smpl_to_model, const double* d_root_offset, int32_t n_models,
                            const double* d_in, const char* in_name, const double* d_trans, int64_t n_frames, const int32_t* d_clip_start,
                            const int32_t* d_clip_model, int32_t n_clips, double* d_qpos, double* d_qpos_quat) {
    // every check comes before the first HIP call
    REFUSE(fn, n_joint != UHC_SC_NJ, "n_joint must be 24 (the SMPL layout: rows of 76 and 99)");
    REFUSE(fn, !h_smpl_to_model, "h_smpl_to_model is NULL");
    REFUSE(fn, !d_in, std::string(in_name) + " is NULL");
    REFUSE(fn, six && ((uintptr_t)d_in & 7), std::string(in_name) + " is not 8-byte aligned");
    REFUSE(fn, !d_clip_start, "d_clip_start is NULL");
    REFUSE(fn, !d_qpos && !d_qpos_quat, "d_qpos and d_qpos_quat are both NULL: nothing to write");
    REFUSE(fn, n_frames < 0, "n_frames < 0");
    REFUSE(fn, n_clips <= 0, "n_clips <= 0");
    REFUSE(fn, n_models <= 0, "n_models <= 0");
    // (d_clip_model NULL: model 0 for every clip, as in uhc_expert_frames; the rows go out in 16-byte stores)
    REFUSE(fn, (uintptr_t)d_qpos & 15, "d_qpos is not 16-byte aligned");
    REFUSE(fn, (uintptr_t)d_qpos_quat & 15, "d_qpos_quat is not 16-byte aligned");
    SmplArgs A = {};
    if (pack_slot_table(fn, h_smpl_to_model, A.slot)) return 1;
    const long long blocks = ((long long)n_frames + SC_FRAMES - 1) / SC_FRAMES;
    REFUSE(fn, !uhc_launch_fits(blocks), "n_frames is beyond one launch (2^34 frames)");
    if (n_frames == 0) return 0;
    A.pose = d_in, A.trans = d_trans, A.root_offset = d_root_offset, A.clip_start = d_clip_start, A.clip_model = d_clip_model;
    A.qpos = d_qpos, A.qpos_quat = d_qpos_quat;
    A.n_frames = n_frames, A.n_clips = n_clips, A.n_models = n_models;
    if (six) hipLaunchKernelGGL(uhc_smpl6d_qpos_kernel, dim3((unsigned)blocks), dim3(SC_THREADS), 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(uhc_smpl_qpos_kernel, dim3((unsigned)blocks), dim3(SC_THREADS), 0, (hipStream_t)stream, A);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int32_t uhc_smpl_qpos(void* stream, int32_t n_joint, const int32_t* h_smpl_to_model, const double* d_root_offset, int32_t n_models,
                                 const double* d_pose_aa, const double* d_trans, int64_t n_frames, const int32_t* d_clip_start, const int32_t* d_clip_model,
                                 int32_t n_clips, double* d_qpos, double* d_qpos_quat) {
    return smpl_qpos_launch("uhc_smpl_qpos", false, stream, n_joint, h_smpl_to_model, d_root_offset, n_models, d_pose_aa, "d_pose_aa", d_trans, n_frames, d_clip_start,
                            d_clip_model, n_clips, d_qpos, d_qpos_quat);
}

extern "C" int32_t uhc_smpl6d_qpos(void* stream, int32_t n_joint, const int32_t* h_smpl_to_model, const double* d_root_offset, int32_t n_models,
                                   const double* d_full_6d, int64_t n_frames, const int32_t* d_clip_start, const int32_t* d_clip_model, int32_t n_clips,
                                   double* d_qpos, double* d_qpos_quat) {
    return smpl_qpos_launch("uhc_smpl6d_qpos", true, stream, n_joint, h_smpl_to_model, d_root_offset, n_models, d_full_6d, "d_full_6d", nullptr, n_frames, d_clip_start,
                            d_clip_model, n_clips, d_qpos, d_qpos_quat);
}

extern "C" int32_t uhc_qpos_smpl(void* stream, int32_t n_joint, const int32_t* h_smpl_to_model, int32_t ball, const double* d_root_offset, int32_t n_models,
                                 const double* d_qpos, int64_t row_stride, int32_t n_seq, int32_t row_cap, const int32_t* d_seq_rows, const int32_t* d_seq_model,
                                 double* d_pose_aa, double* d_trans, double* d_full_6d, int32_t* d_bad, int32_t* h_bad) {
    const char* fn = "uhc_qpos_smpl";
    // every check comes before the first HIP call
    REFUSE(fn, n_joint != UHC_SC_NJ, "n_joint must be 24 (the SMPL layout: rows of 76 and 99)");
    REFUSE(fn, !h_smpl_to_model, "h_smpl_to_model is NULL");
    REFUSE(fn, ball != 0 && ball != 1, "ball must be 0 (hinge rows) or 1 (ball-joint rows)");
    REFUSE(fn, !d_qpos, "d_qpos is NULL");
    REFUSE(fn, (uintptr_t)d_qpos & 7, "d_qpos is not 8-byte aligned");
    const int width = ball ? UHC_SC_NQ_QUAT : UHC_SC_NQ;
    REFUSE(fn, row_stride < width, "row_stride is below the row's width (76 doubles; 99 for ball-joint rows)");
    REFUSE(fn, row_stride > (1LL << 31), "row_stride is beyond 2^31");
    REFUSE(fn, n_seq < 0, "n_seq < 0");
    REFUSE(fn, row_cap <= 0, "row_cap <= 0");
    REFUSE(fn, n_models <= 0, "n_models <= 0");
    REFUSE(fn, !d_pose_aa && !d_trans && !d_full_6d, "d_pose_aa, d_trans and d_full_6d are all NULL: nothing to write");
    REFUSE(fn, (uintptr_t)d_pose_aa & 15, "d_pose_aa is not 16-byte aligned");
    REFUSE(fn, (uintptr_t)d_trans & 15, "d_trans is not 16-byte aligned");
    REFUSE(fn, (uintptr_t)d_full_6d & 15, "d_full_6d is not 16-byte aligned");
    REFUSE(fn, !d_bad, "d_bad is NULL");
    // (d_seq_rows NULL: every row of every sequence; d_seq_model NULL: model 0; d_root_offset NULL: count_offset=False)
    PoseArgs A = {};
    if (pack_slot_table(fn, h_smpl_to_model, A.slot)) return 1;
    const long long n_rows = (long long)n_seq * row_cap, blocks = (n_rows + SC_FRAMES - 1) / SC_FRAMES;
    REFUSE(fn, !uhc_launch_fits(blocks), "n_seq x row_cap is beyond one launch (2^34 rows)");
    if (n_rows == 0) {
        if (h_bad) *h_bad = 0;
        return 0;
    }
    hipStream_t s = (hipStream_t)stream;
    A.qpos = d_qpos, A.root_offset = d_root_offset, A.seq_rows = d_seq_rows, A.seq_model = d_seq_model;
    A.pose_aa = d_pose_aa, A.trans = d_trans, A.full_6d = d_full_6d, A.bad = d_bad;
    A.stride = row_stride, A.n_rows = n_rows, A.row_cap = row_cap, A.n_models = n_models, A.ball = ball;
    A.vec_in = !(row_stride & 1) && !((uintptr_t)d_qpos & 15);  // every row 16-byte aligned: 16-byte loads
    HIP_OK(hipMemsetAsync(d_bad, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(uhc_qpos_smpl_kernel, dim3((unsigned)blocks), dim3(SC_THREADS), 0, s, A);
    HIP_OK(hipGetLastError());
    return uhc_return_bad(h_bad, d_bad, s);
}
