// uhc_eval_metrics.h -- the per-row arithmetic of the imitation metrics (uhc_amd/smpllib/smpl_eval.py: compute_metrics, p_mpjpe; reference:
// uhc/smpllib/smpl_eval.py:24-126), shared by the device kernel (uhc_eval.hip: lane = joint) and a host build (tests/eval_metrics_probe.cpp: a loop over
// the joints).  Everything here is straight-line float64 on fixed-size values: no run-time array index, no allocation, nothing of the HIP runtime.
//
// What is shared are the PIECES between two sums over the 24 joints; the sums themselves belong to the caller (a wave reduction on the device, a loop on
// the host -- uhc_em_row_serial below, the restatement the CPU test runs):
//   uhc_em_root_err       |I - Mp inv(Mg)|_F of the two root transforms
//   uhc_em_joint_norms    one joint's |pred - gt| terms: global, root-relative, velocity, acceleration
//   uhc_em_procrustes     from the centred, normalised clouds' 3 x 3 covariance: rotation, scale, translation (a hand-written SVD: uhc_em_svd3)
//   uhc_em_aligned_err    one joint's distance after that alignment
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define UHC_EM_HD __host__ __device__ __forceinline__
#else
#define UHC_EM_HD inline
#endif
#if defined(__clang__)
#define UHC_EM_UNROLL _Pragma("unroll")
#else
#define UHC_EM_UNROLL
#endif

#define UHC_EM_NJ 24       // joints of a row: bodies 1 .. 24 of xpos, UHC_FR_WBPOS of a bank frame
#define UHC_EM_NMETRIC 6   // root_dist, vel_dist, accel_dist, mpjpe_g, pa_mpjpe, mpjpe: the order of a d_row_metrics row
enum { UHC_EM_ROOT_DIST = 0, UHC_EM_VEL_DIST = 1, UHC_EM_ACCEL_DIST = 2, UHC_EM_MPJPE_G = 3, UHC_EM_PA_MPJPE = 4, UHC_EM_MPJPE = 5 };

struct UhcEmV3 {
    double x, y, z;
};

UHC_EM_HD double uhc_em_norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// quaternion_matrix(q)[:3, :3] (utils/transformation.py): normalises, and is the identity below |q|^2 = 4 eps
UHC_EM_HD void uhc_em_quat_matrix(const double* q, double (&R)[9]) {
    const double n = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    const bool tiny = n < 4.0 * 2.220446049250313e-16;  // (selected, not branched: the matrix stays in registers on the device)
    const double k = tiny ? 0.0 : sqrt(2.0 / n);
    const double w = q[0] * k, x = q[1] * k, y = q[2] * k, z = q[3] * k;
    R[0] = 1.0 - y * y - z * z, R[1] = x * y - z * w, R[2] = x * z + y * w;
    R[3] = x * y + z * w, R[4] = 1.0 - x * x - z * z, R[5] = y * z - x * w;
    R[6] = x * z - y * w, R[7] = y * z + x * w, R[8] = 1.0 - x * x - y * y;
}

// sqrt(sum((I4 - Mp inv(Mg))^2)) for the root transforms of a pred and a gt qpos row (position 0:3, quaternion 3:7).  Mg's rotation block is a rotation by
// construction (quaternion_matrix normalises), so inv(Mg) = [Rg^T, -Rg^T tg]: Mp inv(Mg) = [Rp Rg^T, tp - Rp Rg^T tg]; the last row of the difference is zero.
UHC_EM_HD double uhc_em_root_err(const double* p7, const double* g7) {
    double Rp[9], Rg[9], E[9];
    uhc_em_quat_matrix(p7 + 3, Rp);
    uhc_em_quat_matrix(g7 + 3, Rg);
    double s = 0.0;
UHC_EM_UNROLL
    for (int i = 0; i < 3; i++)
UHC_EM_UNROLL
        for (int j = 0; j < 3; j++) {
            E[3 * i + j] = Rp[3 * i] * Rg[3 * j] + Rp[3 * i + 1] * Rg[3 * j + 1] + Rp[3 * i + 2] * Rg[3 * j + 2];
            const double d = (i == j ? 1.0 : 0.0) - E[3 * i + j];
            s += d * d;
        }
UHC_EM_UNROLL
    for (int i = 0; i < 3; i++) {
        const double d = p7[i] - (E[3 * i] * g7[0] + E[3 * i + 1] * g7[1] + E[3 * i + 2] * g7[2]);
        s += d * d;
    }
    return sqrt(s);
}

struct UhcEmJoint {
    double g, m, vel, acc;  // |p - g|, |(p - p_root) - (g - g_root)|, velocity and acceleration differences (valid where the caller has rows t + 1, t + 2)
    UhcEmV3 p0, g0;         // root-relative pred / gt position: the Procrustes clouds Y (predicted) and X (target)
};

// one joint of row t: p[k], g[k] = its pred / gt position in rows t + k (k = 1, 2 are read only into vel / acc: pass anything where the row does not exist)
UHC_EM_HD UhcEmJoint uhc_em_joint_norms(const UhcEmV3 (&p)[3], const UhcEmV3 (&g)[3], const UhcEmV3& p_root, const UhcEmV3& g_root) {
    UhcEmJoint o;
    o.g = uhc_em_norm3(p[0].x - g[0].x, p[0].y - g[0].y, p[0].z - g[0].z);
    o.p0 = {p[0].x - p_root.x, p[0].y - p_root.y, p[0].z - p_root.z};
    o.g0 = {g[0].x - g_root.x, g[0].y - g_root.y, g[0].z - g_root.z};
    o.m = uhc_em_norm3(o.p0.x - o.g0.x, o.p0.y - o.g0.y, o.p0.z - o.g0.z);
    o.vel = uhc_em_norm3((g[1].x - g[0].x) - (p[1].x - p[0].x), (g[1].y - g[0].y) - (p[1].y - p[0].y), (g[1].z - g[0].z) - (p[1].z - p[0].z));
    o.acc = uhc_em_norm3((g[0].x - 2.0 * g[1].x + g[2].x) - (p[0].x - 2.0 * p[1].x + p[2].x), (g[0].y - 2.0 * g[1].y + g[2].y) - (p[0].y - 2.0 * p[1].y + p[2].y),
                         (g[0].z - 2.0 * g[1].z + g[2].z) - (p[0].z - 2.0 * p[1].z + p[2].z));
    return o;
}

// one Jacobi rotation of the symmetric 3 x 3 matrix in the (p, q) plane; r is the third index; vp, vq the two columns of the accumulated V
UHC_EM_HD void uhc_em_jacobi_rot(double& app, double& aqq, double& apq, double& apr, double& aqr, double (&vp)[3], double (&vq)[3]) {
    // an element that is already negligible beside its diagonal is set to zero and skipped: with theta = (aqq - app) / 2 apq, theta^2 overflows first
    if (!(fabs(apq) > 1e-20 * (fabs(app) + fabs(aqq)))) {
        apq = 0.0;
        return;
    }
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double r0 = apr, r1 = aqr;
    apr = c * r0 - s * r1;
    aqr = s * r0 + c * r1;
UHC_EM_UNROLL
    for (int k = 0; k < 3; k++) {
        const double a = vp[k], b = vq[k];
        vp[k] = c * a - s * b;
        vq[k] = s * a + c * b;
    }
}

// H = U diag(s) V^T, s descending (row-major 3 x 3; U and V hold their vectors in COLUMNS): cyclic Jacobi on H^T H for V, then u_k = H v_k / |H v_k| with
// s_k = |H v_k| (more accurate for a small s_k than the root of the eigenvalue).  A vanishing third singular value (a planar cloud) leaves u_2 undefined:
// it is then u_0 x u_1 -- either sign gives the same rotation after p_mpjpe's determinant fix.
UHC_EM_HD void uhc_em_svd3(const double (&H)[9], double (&U)[9], double (&s)[3], double (&V)[9]) {
    double a00 = H[0] * H[0] + H[3] * H[3] + H[6] * H[6], a01 = H[0] * H[1] + H[3] * H[4] + H[6] * H[7], a02 = H[0] * H[2] + H[3] * H[5] + H[6] * H[8];
    double a11 = H[1] * H[1] + H[4] * H[4] + H[7] * H[7], a12 = H[1] * H[2] + H[4] * H[5] + H[7] * H[8], a22 = H[2] * H[2] + H[5] * H[5] + H[8] * H[8];
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
    for (int sweep = 0; sweep < 30; sweep++) {  // (quadratic convergence: 5 .. 7 sweeps in practice)
        uhc_em_jacobi_rot(a00, a11, a01, a02, a12, v0, v1);
        uhc_em_jacobi_rot(a00, a22, a02, a01, a12, v0, v2);
        uhc_em_jacobi_rot(a11, a22, a12, a01, a02, v1, v2);
        if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
    }
    // descending order of the eigenvalues: three compare-and-swaps
#define UHC_EM_SWAP1(a, b) \
    {                      \
        const double t_ = a; \
        a = b, b = t_;     \
    }
#define UHC_EM_SWAP(la, lb, va, vb)    \
    if (la < lb) {                     \
        UHC_EM_SWAP1(la, lb)           \
        UHC_EM_SWAP1(va[0], vb[0])     \
        UHC_EM_SWAP1(va[1], vb[1])     \
        UHC_EM_SWAP1(va[2], vb[2])     \
    }
    UHC_EM_SWAP(a00, a11, v0, v1)
    UHC_EM_SWAP(a00, a22, v0, v2)
    UHC_EM_SWAP(a11, a22, v1, v2)
#undef UHC_EM_SWAP
#undef UHC_EM_SWAP1
    double u0[3], u1[3], u2[3];
UHC_EM_UNROLL
    for (int i = 0; i < 3; i++) {
        u0[i] = H[3 * i] * v0[0] + H[3 * i + 1] * v0[1] + H[3 * i + 2] * v0[2];
        u1[i] = H[3 * i] * v1[0] + H[3 * i + 1] * v1[1] + H[3 * i + 2] * v1[2];
        u2[i] = H[3 * i] * v2[0] + H[3 * i + 1] * v2[1] + H[3 * i + 2] * v2[2];
    }
    s[0] = uhc_em_norm3(u0[0], u0[1], u0[2]);
    s[1] = uhc_em_norm3(u1[0], u1[1], u1[2]);
    s[2] = uhc_em_norm3(u2[0], u2[1], u2[2]);
UHC_EM_UNROLL
    for (int i = 0; i < 3; i++) u0[i] /= s[0], u1[i] /= s[1];
    if (s[2] > 1e-14 * s[0]) {
UHC_EM_UNROLL
        for (int i = 0; i < 3; i++) u2[i] /= s[2];
    } else {
        u2[0] = u0[1] * u1[2] - u0[2] * u1[1], u2[1] = u0[2] * u1[0] - u0[0] * u1[2], u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
    }
UHC_EM_UNROLL
    for (int i = 0; i < 3; i++) {
        U[3 * i] = u0[i], U[3 * i + 1] = u1[i], U[3 * i + 2] = u2[i];
        V[3 * i] = v0[i], V[3 * i + 1] = v1[i], V[3 * i + 2] = v2[i];
    }
}

struct UhcEmAlign {
    double R[9], a;  // predicted @ R, scaled by a ...
    UhcEmV3 t;       // ... plus t lies on the target
};

// p_mpjpe's alignment from H = X0^T Y0 (X = target = gt, Y = predicted; both centred by muX / muY and divided by their Frobenius norms normX / normY):
// R = V U^T, the determinant fix on V's last column and the last singular value, a = sum(s) normX / normY, t = muX - a muY R
UHC_EM_HD UhcEmAlign uhc_em_procrustes(const double (&H)[9], double normX, double normY, const UhcEmV3& muX, const UhcEmV3& muY) {
    double U[9], s[3], V[9];
    uhc_em_svd3(H, U, s, V);
    UhcEmAlign o;
UHC_EM_UNROLL
    for (int i = 0; i < 3; i++)
UHC_EM_UNROLL
        for (int j = 0; j < 3; j++) o.R[3 * i + j] = V[3 * i] * U[3 * j] + V[3 * i + 1] * U[3 * j + 1] + V[3 * i + 2] * U[3 * j + 2];
    const double det = o.R[0] * (o.R[4] * o.R[8] - o.R[5] * o.R[7]) - o.R[1] * (o.R[3] * o.R[8] - o.R[5] * o.R[6]) + o.R[2] * (o.R[3] * o.R[7] - o.R[4] * o.R[6]);
    const double sign = det > 0.0 ? 1.0 : (det < 0.0 ? -1.0 : det);  // np.sign: 0 stays 0, a NaN a NaN
    V[2] *= sign, V[5] *= sign, V[8] *= sign;
    s[2] *= sign;
UHC_EM_UNROLL
    for (int i = 0; i < 3; i++)
UHC_EM_UNROLL
        for (int j = 0; j < 3; j++) o.R[3 * i + j] = V[3 * i] * U[3 * j] + V[3 * i + 1] * U[3 * j + 1] + V[3 * i + 2] * U[3 * j + 2];
    o.a = (s[0] + s[1] + s[2]) * normX / normY;
    o.t = {muX.x - o.a * (muY.x * o.R[0] + muY.y * o.R[3] + muY.z * o.R[6]), muX.y - o.a * (muY.x * o.R[1] + muY.y * o.R[4] + muY.z * o.R[7]),
           muX.z - o.a * (muY.x * o.R[2] + muY.y * o.R[5] + muY.z * o.R[8])};
    return o;
}

// |a (p0 @ R) + t - g0| of one joint
UHC_EM_HD double uhc_em_aligned_err(const UhcEmAlign& A, const UhcEmV3& p0, const UhcEmV3& g0) {
    return uhc_em_norm3(A.a * (p0.x * A.R[0] + p0.y * A.R[3] + p0.z * A.R[6]) + A.t.x - g0.x, A.a * (p0.x * A.R[1] + p0.y * A.R[4] + p0.z * A.R[7]) + A.t.y - g0.y,
                        A.a * (p0.x * A.R[2] + p0.y * A.R[5] + p0.z * A.R[8]) + A.t.z - g0.z);
}

// One row, the sums over the joints as plain loops in joint order: what the device kernel computes with lane = joint.  pq / gq: the row's pred / gt qpos (7
// numbers read); pj[k] / gj[k]: [72] joint positions of rows t + k (k < n_next + 1; n_next = how many of the rows t + 1, t + 2 exist: 0, 1 or 2).
// out[6] in mm; out[VEL_DIST] / out[ACCEL_DIST] are written only where their rows exist; root_dist is divided by n_rows (compute_metrics' `/ T`).
UHC_EM_HD void uhc_em_row_serial(const double* pq, const double* gq, const double* const (&pj)[3], const double* const (&gj)[3], int n_next, int n_rows, double* out) {
    UhcEmJoint J[UHC_EM_NJ];
    double sg = 0.0, sm = 0.0, sv = 0.0, sa = 0.0;
    UhcEmV3 muX = {0.0, 0.0, 0.0}, muY = {0.0, 0.0, 0.0};
    const UhcEmV3 pr = {pj[0][0], pj[0][1], pj[0][2]}, gr = {gj[0][0], gj[0][1], gj[0][2]};
    for (int j = 0; j < UHC_EM_NJ; j++) {
        UhcEmV3 p[3], g[3];
        for (int k = 0; k < 3; k++) {
            const int kk = k <= n_next ? k : 0;
            p[k] = {pj[kk][3 * j], pj[kk][3 * j + 1], pj[kk][3 * j + 2]};
            g[k] = {gj[kk][3 * j], gj[kk][3 * j + 1], gj[kk][3 * j + 2]};
        }
        J[j] = uhc_em_joint_norms(p, g, pr, gr);
        sg += J[j].g, sm += J[j].m, sv += J[j].vel, sa += J[j].acc;
        muX.x += J[j].g0.x, muX.y += J[j].g0.y, muX.z += J[j].g0.z;
        muY.x += J[j].p0.x, muY.y += J[j].p0.y, muY.z += J[j].p0.z;
    }
    muX = {muX.x / UHC_EM_NJ, muX.y / UHC_EM_NJ, muX.z / UHC_EM_NJ};
    muY = {muY.x / UHC_EM_NJ, muY.y / UHC_EM_NJ, muY.z / UHC_EM_NJ};
    double nX = 0.0, nY = 0.0;
    for (int j = 0; j < UHC_EM_NJ; j++) {
        const UhcEmV3 x0 = {J[j].g0.x - muX.x, J[j].g0.y - muX.y, J[j].g0.z - muX.z}, y0 = {J[j].p0.x - muY.x, J[j].p0.y - muY.y, J[j].p0.z - muY.z};
        nX += x0.x * x0.x + x0.y * x0.y + x0.z * x0.z;
        nY += y0.x * y0.x + y0.y * y0.y + y0.z * y0.z;
    }
    nX = sqrt(nX), nY = sqrt(nY);
    double H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < UHC_EM_NJ; j++) {
        const double x[3] = {(J[j].g0.x - muX.x) / nX, (J[j].g0.y - muX.y) / nX, (J[j].g0.z - muX.z) / nX};
        const double y[3] = {(J[j].p0.x - muY.x) / nY, (J[j].p0.y - muY.y) / nY, (J[j].p0.z - muY.z) / nY};
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) H[3 * a + b] += x[a] * y[b];
    }
    const UhcEmAlign A = uhc_em_procrustes(H, nX, nY, muX, muY);
    double sp = 0.0;
    for (int j = 0; j < UHC_EM_NJ; j++) sp += uhc_em_aligned_err(A, J[j].p0, J[j].g0);
    out[UHC_EM_ROOT_DIST] = uhc_em_root_err(pq, gq) / n_rows * 1000.0;
    if (n_next >= 1) out[UHC_EM_VEL_DIST] = sv / UHC_EM_NJ * 1000.0;
    if (n_next >= 2) out[UHC_EM_ACCEL_DIST] = sa / UHC_EM_NJ * 1000.0;
    out[UHC_EM_MPJPE_G] = sg / UHC_EM_NJ * 1000.0;
    out[UHC_EM_PA_MPJPE] = sp / UHC_EM_NJ * 1000.0;
    out[UHC_EM_MPJPE] = sm / UHC_EM_NJ * 1000.0;
}
