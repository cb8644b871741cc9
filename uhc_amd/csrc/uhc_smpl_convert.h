// uhc_smpl_convert.h -- one joint of the AMASS -> qpos conversion (uhc_amd/smpllib/smpl_mujoco.py: smpl_to_qpose; reference: uhc/smpllib/smpl_mujoco.py:543-607),
// shared by the device kernel (uhc_smpl.hip: one lane per frame and joint) and a host build (tests/smpl_convert_probe.cpp: a loop over the joints).  The per-joint
// pieces are straight-line float64 on fixed-size values: no run-time array index, no allocation, nothing of the HIP runtime.
//
// The host path is scipy's Rotation: from_rotvec, then as_euler("ZYX") (the hinge humanoid), as_quat (the ball-joint humanoid) and as_matrix followed by
// rotation_matrix_to_quaternion (the hinge humanoid's root).  Its arithmetic is restated formula for formula, products and sums rounded separately (no FMA
// contraction), so that host and device differ in the last bits of sqrt / sin / cos / atan2 / hypot alone:
//   uhc_sc_rotvec_quat     rotation vector -> (x, y, z, w), the sign as it comes (no canonical form)
//   uhc_sc_quat_euler_zyx  (x, y, z, w) -> intrinsic ZYX Euler angles (Z, Y, X) by the quaternion algorithm, with its two gimbal-lock branches
//   uhc_sc_quat_matrix     (x, y, z, w) -> rotation matrix
//   uhc_sc_root_quat       rotation matrix -> (w, x, y, z) with the reference converter's branch rule: the branch fixes the sign
//   uhc_sc_row_serial      one frame, the joints as a plain loop: what the device kernel computes with lane = joint
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define UHC_SC_HD __host__ __device__ __forceinline__
#else
#define UHC_SC_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define UHC_SC_NJ 24         // joints of a pose row (SMPL)
#define UHC_SC_NQ 76         // hinge humanoid: root position, root quaternion, 23 x (Z, Y, X)
#define UHC_SC_NQ_QUAT 99    // ball-joint humanoid: root position, 24 x (w, x, y, z)
#define UHC_SC_ROOT_Z 0.91437225  // the root height of a pose that comes without a translation (smpl_to_qpose: trans=None)
#define UHC_SC_PI 3.141592653589793
#define UHC_SC_LOCK_EPS 1e-7      // scipy: the second angle this close to 0 or pi is gimbal lock

struct UhcScQuat {
    double x, y, z, w;  // scipy's order
};
struct UhcScV3 {
    double x, y, z;
};
struct UhcScQ4 {
    double w, x, y, z;  // qpos' order
};
struct UhcScEuler {
    double Z, Y, X;  // as_euler("ZYX")'s order, and the hinge triple's
};

// Rotation.from_rotvec: theta = |r|; below 1e-3 the Taylor series of sin(theta / 2) / theta
UHC_SC_HD UhcScQuat uhc_sc_rotvec_quat(double rx, double ry, double rz) {
    const double angle = sqrt(rx * rx + ry * ry + rz * rz);
    double scale;
    if (angle <= 1e-3) {
        const double angle2 = angle * angle;
        scale = 0.5 - angle2 / 48.0 + angle2 * angle2 / 3840.0;
    } else {
        scale = sin(angle / 2.0) / angle;
    }
    return {scale * rx, scale * ry, scale * rz, cos(angle / 2.0)};
}

UHC_SC_HD double uhc_sc_wrap(double a) { return a < -UHC_SC_PI ? a + 2.0 * UHC_SC_PI : (a > UHC_SC_PI ? a - 2.0 * UHC_SC_PI : a); }

// Rotation.as_euler("ZYX") (intrinsic): the angles about z, then the new y, then the new x.  At lock (Y = -+pi/2) X is 0 and Z takes the whole turn.
UHC_SC_HD UhcScEuler uhc_sc_quat_euler_zyx(const UhcScQuat& q) {
    const double a = q.w - q.y, b = q.x + q.z, c = q.y + q.w, d = q.z - q.x;
    const double beta = 2.0 * atan2(hypot(c, d), hypot(a, b));
    const double half_sum = atan2(b, a), half_diff = atan2(d, c);
    double Z, X;
    if (fabs(beta) <= UHC_SC_LOCK_EPS) {
        Z = 2.0 * half_sum, X = 0.0;
    } else if (fabs(beta - UHC_SC_PI) <= UHC_SC_LOCK_EPS) {
        Z = 2.0 * half_diff, X = 0.0;
    } else {
        Z = half_sum + half_diff, X = half_sum - half_diff;
    }
    return {uhc_sc_wrap(Z), uhc_sc_wrap(beta - UHC_SC_PI / 2.0), uhc_sc_wrap(X)};
}

// Rotation.as_matrix, row-major
UHC_SC_HD void uhc_sc_quat_matrix(const UhcScQuat& q, double (&R)[9]) {
    const double x2 = q.x * q.x, y2 = q.y * q.y, z2 = q.z * q.z, w2 = q.w * q.w;
    const double xy = q.x * q.y, zw = q.z * q.w, xz = q.x * q.z, yw = q.y * q.w, yz = q.y * q.z, xw = q.x * q.w;
    R[0] = x2 - y2 - z2 + w2, R[1] = 2.0 * (xy - zw), R[2] = 2.0 * (xz + yw);
    R[3] = 2.0 * (xy + zw), R[4] = -x2 + y2 - z2 + w2, R[5] = 2.0 * (yz - xw);
    R[6] = 2.0 * (xz - yw), R[7] = 2.0 * (yz + xw), R[8] = -x2 - y2 + z2 + w2;
}

// rotation_matrix_to_quaternion (smpl_mujoco.py): four candidates, chosen by m22 < 1e-6, m00 > m11, m00 < -m11
UHC_SC_HD UhcScQ4 uhc_sc_root_quat(const double (&R)[9]) {
    const double m00 = R[0], m11 = R[4], m22 = R[8];
    double t, w, x, y, z;
    if (m22 < 1e-6) {
        if (m00 > m11) {
            t = 1.0 + m00 - m11 - m22;
            w = R[7] - R[5], x = t, y = R[3] + R[1], z = R[2] + R[6];
        } else {
            t = 1.0 - m00 + m11 - m22;
            w = R[2] - R[6], x = R[3] + R[1], y = t, z = R[7] + R[5];
        }
    } else {
        if (m00 < -m11) {
            t = 1.0 - m00 - m11 + m22;
            w = R[3] - R[1], x = R[2] + R[6], y = R[7] + R[5], z = t;
        } else {
            t = 1.0 + m00 + m11 + m22;
            w = t, x = R[7] - R[5], y = R[2] - R[6], z = R[3] - R[1];
        }
    }
    const double s = sqrt(t);
    return {0.5 * (w / s), 0.5 * (x / s), 0.5 * (y / s), 0.5 * (z / s)};
}

// the root position of a row: the clip's translation (NULL: the default standing height) plus the model's root offset (NULL: count_offset=False)
UHC_SC_HD UhcScV3 uhc_sc_root_pos(const double* trans3, const double* offset3) {
    UhcScV3 p = {0.0, 0.0, UHC_SC_ROOT_Z};
    if (trans3) p = {trans3[0], trans3[1], trans3[2]};
    if (offset3) p = {p.x + offset3[0], p.y + offset3[1], p.z + offset3[2]};
    return p;
}

// One frame, the joints as a plain loop.  pose [72]: the rotation vectors in SMPL joint order; slot_of_joint [24]: the model slot SMPL joint j goes to (the
// inverse of smpl_to_qpose's smpl_2_mujoco table; joint 0 is slot 0).  qpos [76] and / or qpos_quat [99] are written in full, NULL is skipped.
UHC_SC_HD void uhc_sc_row_serial(const double* pose, const double* trans3, const double* offset3, const int* slot_of_joint, double* qpos, double* qpos_quat) {
    const UhcScV3 p = uhc_sc_root_pos(trans3, offset3);
    if (qpos) qpos[0] = p.x, qpos[1] = p.y, qpos[2] = p.z;
    if (qpos_quat) qpos_quat[0] = p.x, qpos_quat[1] = p.y, qpos_quat[2] = p.z;
    for (int j = 0; j < UHC_SC_NJ; j++) {
        const UhcScQuat q = uhc_sc_rotvec_quat(pose[3 * j], pose[3 * j + 1], pose[3 * j + 2]);
        const int m = slot_of_joint[j];
        if (qpos_quat) {
            double* o = qpos_quat + 3 + 4 * m;
            o[0] = q.w, o[1] = q.x, o[2] = q.y, o[3] = q.z;
        }
        if (qpos && j == 0) {
            double R[9];
            uhc_sc_quat_matrix(q, R);
            const UhcScQ4 r = uhc_sc_root_quat(R);
            qpos[3] = r.w, qpos[4] = r.x, qpos[5] = r.y, qpos[6] = r.z;
        } else if (qpos) {
            const UhcScEuler e = uhc_sc_quat_euler_zyx(q);
            double* o = qpos + 7 + 3 * (m - 1);
            o[0] = e.Z, o[1] = e.Y, o[2] = e.X;
        }
    }
}
