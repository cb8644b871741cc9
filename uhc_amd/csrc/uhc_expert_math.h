// uhc_expert_math.h -- one expert frame record from a pair of qpos rows: what uhc_expert.hip (a whole clip bank) and uhc_live.hip (one row per env and control
// step) share.  Humanoid.qpos_fk (uhc_amd/smpllib/torch_smpl_humanoid.py; reference: uhc/smpllib/torch_smpl_humanoid.py:234-261): Euler angles -> joint
// quaternions, forward kinematics, the two finite differences against the neighbouring frame.
//
// Mapping (both kernels): 32 lanes -- a half wave -- per record, lane = body; a body reads its parent's world pose from the parent's lane of its half
// (ds_bpermute), level by level; every field goes into the half's record in LDS.  No arrays are indexed at run time (parents and depths arrive packed in
// kernel-argument words): no scratch.
//
// Arithmetic: uhc_amd/utils/torch_utils.py formula for formula, products and sums rounded separately (no FMA contraction), so that what differs from
// the host path are the last bits of sin / cos / acos alone -- and the two kernels' records of the same rows are the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "uhc_device_env.h"
#include "uhc_seq.h"  // uhc_packed_byte

#pragma clang fp contract(off)

#define XF_NBODY 24
#define XF_NQ 76

// the kinematic tree as kernel-argument words
struct XfTree {
    unsigned long long parent[3];  // h_parent + 1, one byte per body (0 = the root)
    unsigned long long depth[3];   // tree depth, one byte per body
    int ee_body[5];
    int max_depth;
};

// HOST: the live state of an env (uhc_env_live_*): its own bank, one stream of `cap` frames per env.  Owned by the UhcEnv (uhc_env_capi.cpp), whose
// memory stays until uhc_env_free; read by uhc_live.hip's launcher, which packs it into its kernels' arguments.
struct LiveState {
    bool on = false;     // the env is in live mode (uhc_env_live_begin .. uhc_env_live_end / uhc_env_set_bank)
    bool slide = false;  // uhc_env_live_slide; live_begin switches it off
    int cap = 0, alloc_cap = 0, models = 0;
    double dt = 0.0;
    XfTree tree = {};
    double *bank = nullptr, *prev_qpos = nullptr, *beta = nullptr, *body_pos = nullptr, *body_ipos = nullptr;
    int *len = nullptr, *dropped = nullptr, *clip_start = nullptr;
    int *base = nullptr, *moved = nullptr;  // frames slid off / records copied since the restart, per env
};

// HOST: h_parent [24] (the root's parent is -1 and every other parent precedes its child), h_ee_body [5] (0 .. 23) -> T; "" or what is wrong, `who` in front
static inline std::string xf_tree_fill(const char* who, const int32_t* h_parent, const int32_t* h_ee_body, XfTree* T) {
    *T = XfTree{};
    int depth[XF_NBODY];
    for (int i = 0; i < XF_NBODY; i++) {
        const int p = h_parent[i];
        if (i == 0 ? p != -1 : (p < 0 || p >= i))
            return std::string(who) + ": h_parent[" + std::to_string(i) + "] = " + std::to_string(p) +
                   ": the root's parent is -1 and every other parent precedes its child";
        depth[i] = i == 0 ? 0 : depth[p] + 1;
        T->max_depth = depth[i] > T->max_depth ? depth[i] : T->max_depth;
        T->parent[i >> 3] |= (unsigned long long)(p + 1) << (8 * (i & 7));
        T->depth[i >> 3] |= (unsigned long long)depth[i] << (8 * (i & 7));
    }
    for (int k = 0; k < 5; k++) {
        if (h_ee_body[k] < 0 || h_ee_body[k] >= XF_NBODY)
            return std::string(who) + ": h_ee_body[" + std::to_string(k) + "] = " + std::to_string(h_ee_body[k]) + " is outside 0 .. 23";
        T->ee_body[k] = h_ee_body[k];
    }
    return std::string();
}

struct Q4 {
    double w, x, y, z;
};
struct V3 {
    double x, y, z;
};

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

// One half wave, one record.  Called by ALL 64 lanes of a wave (the parent's pose travels by ds_bpermute): `lane` is the lane of the wave, its low five bits the body.
//   row_a, row_b  the difference pair's qpos rows [76]; the record is of row_a when own_is_a, else of row_b.  !paired: no pair -- zero qvel and bangvel
//                 (row_a == row_b then).  Both rows are read by every lane, valid or not: they must be readable.
//   root_record   [4] or NULL: written into the record's qpos[3:7] instead of the own row's quaternion, which kinematics and velocities keep reading
//   body_pos, body_ipos  [24][3] of the record's body shape
//   valid         the half has a record at all: nothing is written to `rec` [UHC_FRAME_STRIDE] (LDS) otherwise
__device__ __forceinline__ void xf_half_record(const XfTree& T, double dt, const double* __restrict__ row_a, const double* __restrict__ row_b, bool own_is_a,
                                               bool paired, const double* __restrict__ root_record, const double* __restrict__ body_pos,
                                               const double* __restrict__ body_ipos, bool valid, int lane, double* rec) {
    const int body = lane & 31;
    const bool has_body = body < XF_NBODY;
    const int bi = has_body ? body : 0;
    // ---- local quaternions of the body in both frames of the pair: the trigonometric half of the work, on 48 lanes
    Q4 qa, qb;
    V3 ang, angb;  // (the root lane keeps the root position here)
    local_quat(row_a, bi, qa, ang);
    local_quat(row_b, bi, qb, angb);
    const Q4 q_own = own_is_a ? qa : qb;
    const V3 ang_own = own_is_a ? ang : angb;

    // get_angvel_fd_batch: rotation_from_quaternion(qb (x) qa^-1) / dt, NOT wrapped
    V3 axis;
    double angle;
    axis_angle(qmul(qb, qinv(qa)), axis, angle);
    V3 bangvel = {axis.x * angle / dt, axis.y * angle / dt, axis.z * angle / dt};
    // get_qvel_fd_batch: root -- linear difference, the same axis-angle wrapped to (-pi, pi] in a's root frame; joints -- plain differences
    V3 v0 = {(angb.x - ang.x) / dt, (angb.y - ang.y) / dt, (angb.z - ang.z) / dt}, v1 = {0.0, 0.0, 0.0};
    if (bi == 0) {
        const double pi = 3.141592653589793;
        double an = angle;
        an = an > pi ? an - 2.0 * pi : an;
        an = an < -pi ? an + 2.0 * pi : an;
        v1 = to_root_frame({axis.x * an / dt, axis.y * an / dt, axis.z * an / dt}, qa);
    }
    if (!paired) bangvel = v0 = v1 = {0.0, 0.0, 0.0};

    // ---- forward_kinematics_batch, level by level: world pose of the parent from the parent's lane (of the same half)
    const int par = uhc_packed_byte(T.parent, bi) - 1, dep = uhc_packed_byte(T.depth, bi);
    const int par_lane = (lane & 32) + (par < 0 ? 0 : par);
    const double* off = body_pos + (size_t)bi * 3;
    const double* ioff = body_ipos + (size_t)bi * 3;
    const V3 o = {off[0], off[1], off[2]}, io = {ioff[0], ioff[1], ioff[2]};
    Q4 wq = q_own;   // (the root's world pose is its qpos; the others are overwritten in their round)
    V3 wp = ang_own;
    for (int d = 1; d <= T.max_depth; d++) {
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
        const double* own_row = own_is_a ? row_a : row_b;
        // (the record's root quaternion may be overridden -- the ball-joint humanoid's second conversion --; everything above read the row's own)
        for (int j = body; j < XF_NQ; j += 32) rec[UHC_FR_QPOS + j] = root_record && j >= 3 && j < 7 ? root_record[j - 3] : own_row[j];
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
                if (body == T.ee_body[k]) {
                    p = rec + UHC_FR_EE + 3 * k;
                    p[0] = wp.x, p[1] = wp.y, p[2] = wp.z;
                }
        }
    }
}
