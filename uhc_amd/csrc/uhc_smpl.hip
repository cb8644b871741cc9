// AMASS axis-angle poses -> qpos rows, computed on the device: uhc_smpl_qpos (include/uhc_amd.h).
//
// The step in front of uhc_expert_frames: smpl_to_qpose (uhc_amd/smpllib/smpl_mujoco.py; reference: uhc/smpllib/smpl_mujoco.py:543-607) is a pure map over
// (frame, joint) -- rotation vector -> quaternion -> intrinsic ZYX Euler angles (the hinge humanoid) or the quaternion itself (the ball-joint humanoid) --,
// reordered from SMPL joint order to the model's depth-first body order.  A frame reads 576 B of pose and 24 B of translation and writes 608 B and / or 792 B.
//
// Mapping: one lane per (frame, SMPL joint), 24 lanes a frame, SC_FRAMES frames a workgroup (a frame's lanes may sit in two waves: no lane talks to another).
//   lane (f, j)     reads joint j's 24 bytes -- a workgroup's lanes read one run of consecutive addresses --, forms the quaternion and from it the hinge triple
//                   and / or the (w, x, y, z) quadruple in registers, and puts them into slot slot_of_joint[j] of the frame's row(s) in LDS.
//   lane (f, 0)     also forms the root quaternion of the 76-wide row (through the rotation matrix: the branch rule that fixes its sign) and the root position:
//                   trans + root_offset[model of the frame's clip]; the clip is the lane's own binary search in d_clip_start, as in uhc_expert.hip.
//   all lanes       copy the workgroup's rows out, 16 B per lane to consecutive addresses.  A workgroup starts at an even frame, so its rows start 16-byte
//                   aligned (8 x 608 B, 8 x 792 B); an odd number of 99-wide rows (the bank's tail) ends in one 8-byte store.
// No array is indexed at run time by a value read from memory: the slot table arrives packed in kernel-argument words (checked on the host to be a
// permutation), a clip's model index is range-checked before it selects a root offset.  No atomics; no scratch.
//
// Arithmetic: uhc_smpl_convert.h, scipy's formulas one for one, products and sums rounded separately (no FMA contraction), so that what differs from the
// host path are the last bits of sqrt / sin / cos / atan2 / hypot alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uhc_amd.h"
#include "uhc_smpl_convert.h"

#include <string>

#pragma clang fp contract(off)

#define SC_FRAMES 8                        // frames per workgroup (even: see above)
#define SC_THREADS (SC_FRAMES * UHC_SC_NJ)  // 192: three waves

extern "C" int uhc_internal_set_error(const char* msg);
#define HIP_OK(expr)                                                                                                          \
    do {                                                                                                                      \
        hipError_t e__ = (expr);                                                                                              \
        if (e__ != hipSuccess) return uhc_internal_set_error((std::string(#expr) + ": " + hipGetErrorString(e__)).c_str()); \
    } while (0)

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

__device__ __forceinline__ int packed_byte(const unsigned long long (&w)[3], int i) {
    const unsigned long long v = i < 8 ? w[0] : (i < 16 ? w[1] : w[2]);
    return (int)((v >> (8 * (i & 7))) & 0xff);
}

__global__ void __launch_bounds__(SC_THREADS) uhc_smpl_qpos_kernel(const SmplArgs A) {
    __shared__ __attribute__((aligned(16))) double row_s[SC_FRAMES * UHC_SC_NQ];        // the workgroup's 76-wide rows, one behind the other as in d_qpos
    __shared__ __attribute__((aligned(16))) double quat_s[SC_FRAMES * UHC_SC_NQ_QUAT];  // ... and its 99-wide rows
    const int tid = threadIdx.x, fl = tid / UHC_SC_NJ, j = tid - fl * UHC_SC_NJ;
    const long long f0 = (long long)blockIdx.x * SC_FRAMES, f = f0 + fl;
    if (f < A.n_frames) {
        const double* r = A.pose + (size_t)f * (3 * UHC_SC_NJ) + 3 * j;
        const UhcScQuat q = uhc_sc_rotvec_quat(r[0], r[1], r[2]);
        const int m = packed_byte(A.slot, j);  // (a permutation of 0 .. 23 with slot[0] = 0: checked before the launch)
        double* row = row_s + fl * UHC_SC_NQ;
        double* qrow = quat_s + fl * UHC_SC_NQ_QUAT;
        if (A.qpos_quat) {
            double* o = qrow + 3 + 4 * m;
            o[0] = q.w, o[1] = q.x, o[2] = q.y, o[3] = q.z;
        }
        if (j == 0) {
            // ---- the frame's clip: the last clip whose start is <= f; all it decides is which model's root offset the row gets
            const double* off = nullptr;
            if (A.root_offset) {
                int lo = 0, hi = A.n_clips - 1;
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if ((long long)A.clip_start[mid] <= f) lo = mid;
                    else hi = mid - 1;
                }
                // (lo stays inside the table whatever it holds: a table that is not ascending can name the wrong clip, never an address outside the arrays)
                int mi = A.clip_model ? A.clip_model[lo] : 0;
                mi = mi < 0 || mi >= A.n_models ? 0 : mi;
                off = A.root_offset + (size_t)mi * 3;
            }
            const UhcScV3 p = uhc_sc_root_pos(A.trans ? A.trans + (size_t)f * 3 : nullptr, off);
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

// ------------------------------------------------------------------ C-ABI (include/uhc_amd.h)
extern "C" int32_t uhc_smpl_qpos(void* stream, int32_t n_joint, const int32_t* h_smpl_to_model, const double* d_root_offset, int32_t n_models,
                                 const double* d_pose_aa, const double* d_trans, int64_t n_frames, const int32_t* d_clip_start, const int32_t* d_clip_model,
                                 int32_t n_clips, double* d_qpos, double* d_qpos_quat) {
    // every check comes before the first HIP call
    if (n_joint != UHC_SC_NJ) return uhc_internal_set_error("uhc_smpl_qpos: n_joint must be 24 (the SMPL layout: rows of 76 and 99)");
    if (!h_smpl_to_model) return uhc_internal_set_error("uhc_smpl_qpos: h_smpl_to_model is NULL");
    if (!d_pose_aa) return uhc_internal_set_error("uhc_smpl_qpos: d_pose_aa is NULL");
    if (!d_clip_start) return uhc_internal_set_error("uhc_smpl_qpos: d_clip_start is NULL");
    if (!d_qpos && !d_qpos_quat) return uhc_internal_set_error("uhc_smpl_qpos: d_qpos and d_qpos_quat are both NULL: nothing to write");
    if (n_frames < 0) return uhc_internal_set_error("uhc_smpl_qpos: n_frames < 0");
    if (n_clips <= 0) return uhc_internal_set_error("uhc_smpl_qpos: n_clips <= 0");
    if (n_models <= 0) return uhc_internal_set_error("uhc_smpl_qpos: n_models <= 0");
    // (d_clip_model NULL: model 0 for every clip, as in uhc_expert_frames; the rows go out in 16-byte stores)
    if ((uintptr_t)d_qpos & 15) return uhc_internal_set_error("uhc_smpl_qpos: d_qpos is not 16-byte aligned");
    if ((uintptr_t)d_qpos_quat & 15) return uhc_internal_set_error("uhc_smpl_qpos: d_qpos_quat is not 16-byte aligned");
    SmplArgs A = {};
    unsigned seen = 0;
    for (int m = 0; m < UHC_SC_NJ; m++) {
        const int j = h_smpl_to_model[m];
        if (j < 0 || j >= UHC_SC_NJ || (seen >> j & 1u) || (m == 0) != (j == 0))
            return uhc_internal_set_error(("uhc_smpl_qpos: h_smpl_to_model[" + std::to_string(m) + "] = " + std::to_string(j) +
                                           ": the table is a permutation of 0 .. 23 that keeps the root at 0").c_str());
        seen |= 1u << j;
        A.slot[j >> 3] |= (unsigned long long)m << (8 * (j & 7));
    }
    const long long blocks = ((long long)n_frames + SC_FRAMES - 1) / SC_FRAMES;
    if (blocks > 0x7fffffffLL) return uhc_internal_set_error("uhc_smpl_qpos: n_frames is beyond one launch (2^34 frames)");
    if (n_frames == 0) return 0;
    A.pose = d_pose_aa, A.trans = d_trans, A.root_offset = d_root_offset, A.clip_start = d_clip_start, A.clip_model = d_clip_model;
    A.qpos = d_qpos, A.qpos_quat = d_qpos_quat;
    A.n_frames = n_frames, A.n_clips = n_clips, A.n_models = n_models;
    hipLaunchKernelGGL(uhc_smpl_qpos_kernel, dim3((unsigned)blocks), dim3(SC_THREADS), 0, (hipStream_t)stream, A);
    HIP_OK(hipGetLastError());
    return 0;
}
