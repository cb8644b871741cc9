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
//                   and the body shape -- is the lane's own binary search in d_clip_start, so the two halves may sit in different clips.
//                   Then the finite differences, and the tree level by level: a body reads its parent's world pose from the parent's lane of its
//                   half (ds_bpermute), depth <= 23 rounds, 8 on the SMPL tree.  Every field goes into the half's record in LDS.
//   all 64 lanes    copy the wave's two records out, 16 B per lane to consecutive addresses (2 x 292 x 16 B: 9.1 wave-wide stores per wave).
// No arrays are indexed at run time (parents and depths arrive packed in kernel-argument words): the kernel uses no scratch.
//
// Arithmetic: uhc_amd/utils/torch_utils.py formula for formula, products and sums rounded separately (no FMA contraction), so that what differs from
// the host path are the last bits of sin / cos / acos alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uhc_amd.h"
#include "uhc_device_env.h"

#include <string>

#pragma clang fp contract(off)

#define XF_NBODY 24
#define XF_NQ 76
#define XF_WAVES 4  // waves per workgroup: eight frames

extern "C" int uhc_internal_set_error(const char* msg);
#define HIP_OK(expr)                                                                                                          \
    do {                                                                                                                      \
        hipError_t e__ = (expr);                                                                                              \
        if (e__ != hipSuccess) return uhc_internal_set_error((std::string(#expr) + ": " + hipGetErrorString(e__)).c_str()); \
    } while (0)

struct ExpertArgs {
    const double* qpos;         // [n_frames][76]
    const double* root_record;  // [n_frames][4] or NULL
    const int* clip_start;      // [n_clips]
    const int* clip_model;      // [n_clips] or NULL
    const double* body_pos;     // [n_models][24][3]
    const double* body_ipos;    // [n_models][24][3]
    double* frames;             // [n_frames][UHC_FRAME_STRIDE]
    long long n_frames;
    int n_clips, n_models, max_depth;
    double dt;
    unsigned long long parent[3];  // h_parent + 1, one byte per body (0 = the root)
    unsigned long long depth[3];   // tree depth, one byte per body
    int ee_body[5];
};

struct Q4 {
    double w, x, y, z;
};
struct V3 {
    double x, y, z;
};

__device__ __forceinline__ int packed_byte(const unsigned long long (&w)[3], int i) {
    const unsigned long long v = i < 8 ? w[0] : (i < 16 ? w[1] : w[2]);
    return (int)((v >> (8 * (i & 7))) & 0xff);
}

// quaternion_multiply_batch (torch_utils.py)
__device__ __forceinline__ Q4 qmul(const Q4& a, const Q4& b) {
    return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
            a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}

// quaternion_inverse_batch: conjugate / |q|^2
__device__ __forceinline__ Q4 qinv(const Q4& q) {
    const double n = q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z;
    return {q.w / n, -q.x / n, -q.y / n, -q.z / n};
}

// quat_mul_vec_batch: the cross-product form, |q| = 1 assumed
__device__ __forceinline__ V3 qrot(const Q4& q, const V3& v) {
    const V3 uv = {q.y * v.z - q.z * v.y, q.z * v.x - q.x * v.z, q.x * v.y - q.y * v.x};
    const V3 uuv = {q.y * uv.z - q.z * uv.y, q.z * uv.x - q.x * uv.z, q.x * uv.y - q.y * uv.x};
    return {v.x + 2.0 * (q.w * uv.x + uuv.x), v.y + 2.0 * (q.w * uv.y + uuv.y), v.z + 2.0 * (q.w * uv.z + uuv.z)};
}

// rotation_from_quaternion_batch(separate=True): safe_acos' clamp at +-(1 - 1e-7), the |sin| < 1e-5 axis guard
__device__ __forceinline__ void axis_angle(const Q4& q, V3& axis, double& angle) {
    const double c = fmin(fmax(q.w, -1.0 + 1e-7), 1.0 - 1e-7);
    const double half = acos(q.w != q.w ? q.w : c);  // (a NaN stays a NaN, as torch.clamp leaves it)
    const double s = sin(half);
    const bool cond = fabs(s) < 1e-5;
    const double d = cond ? 1.0 : s;
    axis = cond ? V3{1.0, 0.0, 0.0} : V3{q.x / d, q.y / d, q.z / d};
    angle = cond ? 0.0 : 2.0 * half;
}

// transform_vec_batch: R(q)^T v with quaternion_matrix_batch's normalisation
__device__ __forceinline__ V3 to_root_frame(const V3& v, const Q4& q0) {
    const double nrm = sqrt(q0.w * q0.w + q0.x * q0.x + q0.y * q0.y + q0.z * q0.z);
    const double w = q0.w / nrm, x = q0.x / nrm, y = q0.y / nrm, z = q0.z / nrm;
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double r00 = 1.0 - (tyy + tzz), r01 = txy - twz, r02 = txz + twy;
    const double r10 = txy + twz, r11 = 1.0 - (txx + tzz), r12 = tyz - twx;
    const double r20 = txz - twy, r21 = tyz + twx, r22 = 1.0 - (txx + tyy);
    return {r00 * v.x + r10 * v.y + r20 * v.z, r01 * v.x + r11 * v.y + r21 * v.z, r02 * v.x + r12 * v.y + r22 * v.z};
}

__device__ __forceinline__ double clip10(double v) { return v < -10.0 ? -10.0 : (v > 10.0 ? 10.0 : v); }  // (NaN passes, as torch.clip lets it)

__device__ __forceinline__ Q4 shfl_q(const Q4& q, int src) { return {__shfl(q.w, src), __shfl(q.x, src), __shfl(q.y, src), __shfl(q.z, src)}; }
__device__ __forceinline__ V3 shfl_v(const V3& v, int src) { return {__shfl(v.x, src), __shfl(v.y, src), __shfl(v.z, src)}; }

// quaternion_from_euler_rzyx of a body's hinge triple (az, ay, ax), or the root's quaternion as qpos gives it; `ang` keeps the triple (the root: its position)
__device__ __forceinline__ void local_quat(const double* __restrict__ qrow, int bi, Q4& ql, V3& ang) {
    if (bi == 0) {
        ang = {qrow[0], qrow[1], qrow[2]};
        ql = {qrow[3], qrow[4], qrow[5], qrow[6]};
    } else {
        ang = {qrow[7 + 3 * (bi - 1)], qrow[8 + 3 * (bi - 1)], qrow[9 + 3 * (bi - 1)]};
        double sz, cz, sy, cy, sx, cx;
        sincos(ang.x / 2.0, &sz, &cz);
        sincos(ang.y / 2.0, &sy, &cy);
        sincos(ang.z / 2.0, &sx, &cx);
        ql = {cx * cy * cz + sx * sy * sz, sx * cy * cz - cx * sy * sz, cx * sy * cz + sx * cy * sz, cx * cy * sz - sx * sy * cz};
    }
}

__global__ void __launch_bounds__(64 * XF_WAVES) uhc_expert_frames_kernel(const ExpertArgs A) {
    __shared__ __attribute__((aligned(16))) double rec_s[2 * XF_WAVES][UHC_FRAME_STRIDE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, body = lane & 31;
    const long long f0 = ((long long)blockIdx.x * XF_WAVES + wave) * 2;  // the wave's frames: f0 (lanes 0 .. 31) and f0 + 1 (lanes 32 .. 63)
    const bool wave_valid = f0 < A.n_frames;                             // (wave-uniform; the barrier below is reached by every wave)
    if (wave_valid) {
        const bool valid = f0 + half < A.n_frames;     // (the bank's last frame may have no partner: that half computes its neighbour's frame along and stores nothing)
        const long long f = valid ? f0 + half : f0;
        double* rec = rec_s[2 * wave + half];
        // ---- the frame's clip: the last clip whose start is <= f (the kernel's own lookup)
        int lo = 0, hi = A.n_clips - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if ((long long)A.clip_start[mid] <= f) lo = mid;
            else hi = mid - 1;
        }
        const long long s = A.clip_start[lo];
        const long long e = lo + 1 < A.n_clips ? (long long)A.clip_start[lo + 1] : A.n_frames;
        // (a table that is not ascending cannot send a read outside [0, n_frames): such a frame is treated as a clip of its own)
        const bool paired = s >= 0 && s <= f && f < e && e <= A.n_frames && e - s >= 2;
        // the difference pair (a, b): (t - 1, t) for frame t >= 1 of a clip, (0, 1) for its frame 0; a clip of one frame has none
        const long long fa = paired ? (f > s ? f - 1 : s) : f, fb = paired ? fa + 1 : f;
        int m = A.clip_model ? A.clip_model[lo] : 0;
        m = m < 0 || m >= A.n_models ? 0 : m;

        const bool has_body = body < XF_NBODY;
        const int bi = has_body ? body : 0;
        // ---- local quaternions of the body in both frames of the pair: the trigonometric half of the work, on 48 lanes
        Q4 qa, qb;
        V3 ang, angb;  // (the root lane keeps the root position here)
        local_quat(A.qpos + (size_t)fa * XF_NQ, bi, qa, ang);
        local_quat(A.qpos + (size_t)fb * XF_NQ, bi, qb, angb);
        const bool own_is_a = f == fa;  // frame 0 of a clip (and an unpaired frame) IS a; every other frame is b
        const Q4 q_own = own_is_a ? qa : qb;
        const V3 ang_own = own_is_a ? ang : angb;

        // get_angvel_fd_batch: rotation_from_quaternion(qb (x) qa^-1) / dt, NOT wrapped
        V3 axis;
        double angle;
        axis_angle(qmul(qb, qinv(qa)), axis, angle);
        V3 bangvel = {axis.x * angle / A.dt, axis.y * angle / A.dt, axis.z * angle / A.dt};
        // get_qvel_fd_batch: root -- linear difference, the same axis-angle wrapped to (-pi, pi] in a's root frame; joints -- plain differences
        V3 v0 = {(angb.x - ang.x) / A.dt, (angb.y - ang.y) / A.dt, (angb.z - ang.z) / A.dt}, v1 = {0.0, 0.0, 0.0};
        if (bi == 0) {
            const double pi = 3.141592653589793;
            double an = angle;
            an = an > pi ? an - 2.0 * pi : an;
            an = an < -pi ? an + 2.0 * pi : an;
            v1 = to_root_frame({axis.x * an / A.dt, axis.y * an / A.dt, axis.z * an / A.dt}, qa);
        }
        if (!paired) bangvel = v0 = v1 = {0.0, 0.0, 0.0};

        // ---- forward_kinematics_batch, level by level: world pose of the parent from the parent's lane (of the same half)
        const int par = packed_byte(A.parent, bi) - 1, dep = packed_byte(A.depth, bi);
        const int par_lane = (lane & 32) + (par < 0 ? 0 : par);
        const double* off = A.body_pos + ((size_t)m * XF_NBODY + bi) * 3;
        const double* ioff = A.body_ipos + ((size_t)m * XF_NBODY + bi) * 3;
        const V3 o = {off[0], off[1], off[2]}, io = {ioff[0], ioff[1], ioff[2]};
        Q4 wq = q_own;   // (the root's world pose is its qpos; the others are overwritten in their round)
        V3 wp = ang_own;
        for (int d = 1; d <= A.max_depth; d++) {
            const Q4 pq = shfl_q(wq, par_lane);
            const V3 pp = shfl_v(wp, par_lane);
            if (dep == d) {
                const V3 r = qrot(pq, o);
                wp = {r.x + pp.x, r.y + pp.y, r.z + pp.z};
                wq = qmul(pq, q_own);
            }
        }
        const V3 rc = qrot(wq, io);
        const V3 com = {rc.x + wp.x, rc.y + wp.y, rc.z + wp.z};

        // ---- the record, in LDS
        if (valid) {
            const double* own_row = A.qpos + (size_t)f * XF_NQ;
            // (the record's root quaternion may be overridden -- the ball-joint humanoid's second conversion --; everything above read d_qpos' own)
            for (int j = body; j < XF_NQ; j += 32)
                rec[UHC_FR_QPOS + j] = A.root_record && j >= 3 && j < 7 ? A.root_record[(size_t)f * 4 + (j - 3)] : own_row[j];
            if (body < 7) rec[UHC_FR_COM + 3 + body] = 0.0;  // slots 505 .. 511
            if (has_body) {
                if (body == 0) {
                    rec[UHC_FR_QVEL + 0] = clip10(v0.x), rec[UHC_FR_QVEL + 1] = clip10(v0.y), rec[UHC_FR_QVEL + 2] = clip10(v0.z);
                    rec[UHC_FR_QVEL + 3] = clip10(v1.x), rec[UHC_FR_QVEL + 4] = clip10(v1.y), rec[UHC_FR_QVEL + 5] = clip10(v1.z);
                    rec[UHC_FR_COM + 0] = com.x, rec[UHC_FR_COM + 1] = com.y, rec[UHC_FR_COM + 2] = com.z;
                } else {
                    double* qv = rec + UHC_FR_QVEL + 6 + 3 * (body - 1);
                    qv[0] = clip10(v0.x), qv[1] = clip10(v0.y), qv[2] = clip10(v0.z);
                }
                double* p = rec + UHC_FR_WBPOS + 3 * body;
                p[0] = wp.x, p[1] = wp.y, p[2] = wp.z;
                p = rec + UHC_FR_WBQUAT + 4 * body;
                p[0] = wq.w, p[1] = wq.x, p[2] = wq.y, p[3] = wq.z;
                p = rec + UHC_FR_BQUAT + 4 * body;
                p[0] = q_own.w, p[1] = q_own.x, p[2] = q_own.y, p[3] = q_own.z;
                p = rec + UHC_FR_BANGVEL + 3 * body;
                p[0] = bangvel.x, p[1] = bangvel.y, p[2] = bangvel.z;
                p = rec + UHC_FR_BCOM + 3 * body;
                p[0] = com.x, p[1] = com.y, p[2] = com.z;
#pragma unroll
                for (int k = 0; k < 5; k++)
                    if (body == A.ee_body[k]) {
                        p = rec + UHC_FR_EE + 3 * k;
                        p[0] = wp.x, p[1] = wp.y, p[2] = wp.z;
                    }
            }
        }
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
    if (n_body != XF_NBODY) return uhc_internal_set_error("uhc_expert_frames: n_body must be 24 (UHC_FRAME_STRIDE is a 24-body layout)");
    if (!h_parent) return uhc_internal_set_error("uhc_expert_frames: h_parent is NULL");
    if (!h_ee_body) return uhc_internal_set_error("uhc_expert_frames: h_ee_body is NULL");
    if (!d_body_pos) return uhc_internal_set_error("uhc_expert_frames: d_body_pos is NULL");
    if (!d_body_ipos) return uhc_internal_set_error("uhc_expert_frames: d_body_ipos is NULL");
    if (!d_qpos) return uhc_internal_set_error("uhc_expert_frames: d_qpos is NULL");
    if (!d_clip_start) return uhc_internal_set_error("uhc_expert_frames: d_clip_start is NULL");
    if (!d_frames) return uhc_internal_set_error("uhc_expert_frames: d_frames is NULL");
    if (n_frames < 0) return uhc_internal_set_error("uhc_expert_frames: n_frames < 0");
    if (n_clips <= 0) return uhc_internal_set_error("uhc_expert_frames: n_clips <= 0");
    if (n_models <= 0) return uhc_internal_set_error("uhc_expert_frames: n_models <= 0");
    if (!(dt > 0.0)) return uhc_internal_set_error("uhc_expert_frames: dt <= 0");
    ExpertArgs A = {};
    int depth[XF_NBODY];
    for (int i = 0; i < XF_NBODY; i++) {
        const int p = h_parent[i];
        if (i == 0 ? p != -1 : (p < 0 || p >= i))
            return uhc_internal_set_error(("uhc_expert_frames: h_parent[" + std::to_string(i) + "] = " + std::to_string(p) +
                                           ": the root's parent is -1 and every other parent precedes its child").c_str());
        depth[i] = i == 0 ? 0 : depth[p] + 1;
        A.max_depth = depth[i] > A.max_depth ? depth[i] : A.max_depth;
        A.parent[i >> 3] |= (unsigned long long)(p + 1) << (8 * (i & 7));
        A.depth[i >> 3] |= (unsigned long long)depth[i] << (8 * (i & 7));
    }
    for (int k = 0; k < 5; k++) {
        if (h_ee_body[k] < 0 || h_ee_body[k] >= XF_NBODY)
            return uhc_internal_set_error(("uhc_expert_frames: h_ee_body[" + std::to_string(k) + "] = " + std::to_string(h_ee_body[k]) + " is outside 0 .. 23").c_str());
        A.ee_body[k] = h_ee_body[k];
    }
    const long long blocks = ((long long)n_frames + 2 * XF_WAVES - 1) / (2 * XF_WAVES);
    if (blocks > 0x7fffffffLL) return uhc_internal_set_error("uhc_expert_frames: n_frames is beyond one launch (2^34 frames)");
    if (n_frames == 0) return 0;
    A.qpos = d_qpos, A.root_record = d_root_quat_record, A.clip_start = d_clip_start, A.clip_model = d_clip_model;
    A.body_pos = d_body_pos, A.body_ipos = d_body_ipos, A.frames = d_frames;
    A.n_frames = n_frames, A.n_clips = n_clips, A.n_models = n_models, A.dt = dt;
    hipLaunchKernelGGL(uhc_expert_frames_kernel, dim3((unsigned)blocks), dim3(64 * XF_WAVES), 0, (hipStream_t)stream, A);
    HIP_OK(hipGetLastError());
    return 0;
}
