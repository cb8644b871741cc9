// Expert frame records of a clip bank, computed on the device: uhc_expert_frames (include/uhc_amd.h).
//
// What the env layer reads per control step is the clip bank, UHC_FRAME_STRIDE doubles per expert frame (uhc_device_env.h).  The records are a pure
// map over frames of Humanoid.qpos_fk (uhc_amd/smpllib/torch_smpl_humanoid.py; reference: uhc/smpllib/torch_smpl_humanoid.py:234-261): Euler angles ->
// joint quaternions, forward kinematics, and the two finite differences against the neighbouring frame of the SAME clip.  A frame reads 2 x 608 B of
// qpos and writes 4 672 B; measured, the kernel is bound by float64 instruction issue at about half of a plain copy's rate.
//
// Mapping: one wave per TWO frames (lanes 0 .. 31 the even one, lanes 32 .. 63 the odd one), four waves per workgroup; within a half, lane = body.
//   lanes b, 32 + b (b < 24)  turn body b's three Euler angles into the joint quaternion for BOTH frames of the half's difference pair (a, b): the pair is
//                   (t - 1, t) for frame t >= 1 of a clip and (0, 1) for its frame 0 -- the cat((qvel[0:1], qvel)) rule --; a clip of ONE frame has
//                   no pair: its qvel and bangvel are zero (the host path cannot compute such a clip at all).  The frame's clip -- and with it the pair
//                   and the body shape -- is the lane's own binary search in d_clip_start (uhc_seq.h: uhc_clip_of), so the two halves may sit in different clips.
//                   Then the finite differences, and the tree level by level: a body reads its parent's world pose from the parent's lane of its
//                   half (ds_bpermute), depth <= 23 rounds, 8 on the SMPL tree.  Every field goes into the half's record in LDS.
//   all 64 lanes    copy the wave's two records out, 16 B per lane to consecutive addresses (2 x 292 x 16 B: 9.1 wave-wide stores per wave).
// No arrays are indexed at run time (parents and depths arrive packed in kernel-argument words): the kernel uses no scratch.
//
// Arithmetic: uhc_amd/utils/torch_utils.py formula for formula, products and sums rounded separately (no FMA contraction), so that what differs from
// the host path are the last bits of sin / cos / acos alone.  The record of one pair of rows -- the per-half body of the kernel -- is uhc_expert_math.h's
// xf_half_record, shared with uhc_live.hip (one row per env and control step); this unit keeps the clip lookup and the copy out of LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uhc_amd.h"
#include "uhc_api_check.h"
#include "uhc_device_env.h"
#include "uhc_expert_math.h"  // the record of one pair of rows, shared with uhc_live.hip
#include "uhc_seq.h"

#pragma clang fp contract(off)

#define XF_WAVES 4  // waves per workgroup: eight frames

struct ExpertArgs {
    const double* qpos;         // [n_frames][76]
    const double* root_record;  // [n_frames][4] or NULL
    const int* clip_start;      // [n_clips]
    const int* clip_model;      // [n_clips] or NULL
    const double* body_pos;     // [n_models][24][3]
    const double* body_ipos;    // [n_models][24][3]
    double* frames;             // [n_frames][UHC_FRAME_STRIDE]
    long long n_frames;
    int n_clips, n_models;
    double dt;
    XfTree tree;
};

__global__ void __launch_bounds__(64 * XF_WAVES) uhc_expert_frames_kernel(const ExpertArgs A) {
    __shared__ __attribute__((aligned(16))) double rec_s[2 * XF_WAVES][UHC_FRAME_STRIDE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
    const long long f0 = ((long long)blockIdx.x * XF_WAVES + wave) * 2;  // the wave's frames: f0 (lanes 0 .. 31) and f0 + 1 (lanes 32 .. 63)
    const bool wave_valid = f0 < A.n_frames;                             // (wave-uniform; the barrier below is reached by every wave)
    if (wave_valid) {
        const bool valid = f0 + half < A.n_frames;     // (the bank's last frame may have no partner: that half computes its neighbour's frame along and stores nothing)
        const long long f = valid ? f0 + half : f0;
        double* rec = rec_s[2 * wave + half];
        const int lo = uhc_clip_of(A.clip_start, A.n_clips, f);  // the frame's clip
        const long long s = A.clip_start[lo];
        const long long e = lo + 1 < A.n_clips ? (long long)A.clip_start[lo + 1] : A.n_frames;
        // (a table that is not ascending cannot send a read outside [0, n_frames): such a frame is treated as a clip of its own)
        const bool paired = s >= 0 && s <= f && f < e && e <= A.n_frames && e - s >= 2;
        // the difference pair (a, b): (t - 1, t) for frame t >= 1 of a clip, (0, 1) for its frame 0; a clip of one frame has none
        const long long fa = paired ? (f > s ? f - 1 : s) : f, fb = paired ? fa + 1 : f;
        const int m = uhc_seq_model(A.clip_model, lo, A.n_models);

        // the record of the pair, in LDS (uhc_expert_math.h); frame 0 of a clip (and an unpaired frame) IS a, every other frame is b
        xf_half_record(A.tree, A.dt, A.qpos + (size_t)fa * XF_NQ, A.qpos + (size_t)fb * XF_NQ, f == fa, paired, A.root_record ? A.root_record + (size_t)f * 4 : nullptr,
                       A.body_pos + (size_t)m * XF_NBODY * 3, A.body_ipos + (size_t)m * XF_NBODY * 3, valid, lane, rec);
    }
    __syncthreads();
    if (wave_valid) {
        // the wave's two records lie one behind the other, in LDS as in the bank: one run of consecutive 16-byte stores
        const int n2 = (f0 + 1 < A.n_frames ? 2 : 1) * (UHC_FRAME_STRIDE / 2);
        const double2* src = reinterpret_cast<const double2*>(rec_s[2 * wave]);
        double2* dst = reinterpret_cast<double2*>(A.frames + (size_t)f0 * UHC_FRAME_STRIDE);  // 4 672 B per record: 16-byte aligned
        for (int j = lane; j < n2; j += 64) dst[j] = src[j];
    }
}

// ------------------------------------------------------------------ C-ABI (include/uhc_amd.h)
extern "C" int32_t uhc_expert_frames(void* stream, int32_t n_body, const int32_t* h_parent, const int32_t* h_ee_body, const double* d_body_pos,
                                     const double* d_body_ipos, int32_t n_models, const double* d_qpos, int64_t n_frames, const int32_t* d_clip_start,
                                     const int32_t* d_clip_model, int32_t n_clips, const double* d_root_quat_record, double dt, double* d_frames) {
    // every check comes before the first HIP call
    REFUSE("uhc_expert_frames", n_body != XF_NBODY, "n_body must be 24 (UHC_FRAME_STRIDE is a 24-body layout)");
    REFUSE("uhc_expert_frames", !h_parent, "h_parent is NULL");
    REFUSE("uhc_expert_frames", !h_ee_body, "h_ee_body is NULL");
    REFUSE("uhc_expert_frames", !d_body_pos, "d_body_pos is NULL");
    REFUSE("uhc_expert_frames", !d_body_ipos, "d_body_ipos is NULL");
    REFUSE("uhc_expert_frames", !d_qpos, "d_qpos is NULL");
    REFUSE("uhc_expert_frames", !d_clip_start, "d_clip_start is NULL");
    REFUSE("uhc_expert_frames", !d_frames, "d_frames is NULL");
    REFUSE("uhc_expert_frames", n_frames < 0, "n_frames < 0");
    REFUSE("uhc_expert_frames", n_clips <= 0, "n_clips <= 0");
    REFUSE("uhc_expert_frames", n_models <= 0, "n_models <= 0");
    REFUSE("uhc_expert_frames", !(dt > 0.0), "dt <= 0");
    ExpertArgs A = {};
    const std::string bad = xf_tree_fill("uhc_expert_frames", h_parent, h_ee_body, &A.tree);
    if (!bad.empty()) return uhc_internal_set_error(bad.c_str());
    const long long blocks = ((long long)n_frames + 2 * XF_WAVES - 1) / (2 * XF_WAVES);
    REFUSE("uhc_expert_frames", !uhc_launch_fits(blocks), "n_frames is beyond one launch (2^34 frames)");
    if (n_frames == 0) return 0;
    A.qpos = d_qpos, A.root_record = d_root_quat_record, A.clip_start = d_clip_start, A.clip_model = d_clip_model;
    A.body_pos = d_body_pos, A.body_ipos = d_body_ipos, A.frames = d_frames;
    A.n_frames = n_frames, A.n_clips = n_clips, A.n_models = n_models, A.dt = dt;
    hipLaunchKernelGGL(uhc_expert_frames_kernel, dim3((unsigned)blocks), dim3(64 * XF_WAVES), 0, (hipStream_t)stream, A);
    HIP_OK(hipGetLastError());
    return 0;
}
