// uhc_surface_math.h -- the per-vertex arithmetic of the surface metrics (penetration, skate, float, contact count: uhc_amd/smpllib/smpl_eval.py:
// compute_penetration, compute_skate, compute_float on hull_vertices; reference: uhc/smpllib/smpl_eval.py:125-149, there on SMPL vertices), shared by the
// device kernel (uhc_surface.hip: the vertices dealt to the lanes) and a host build (tests/surface_metrics_probe.cpp: a loop over the vertices).
// Straight-line float64 on fixed-size values: no run-time array index, no allocation, nothing of the HIP runtime.
//
// What is shared are the PIECES of one vertex; the sums over the vertices belong to the caller (per-lane partial sums and a wave reduction on the device, a
// loop on the host -- uhc_sf_row_serial below, which the CPU test runs); how the finished row is stored is shared again, uhc_sf_store_row:
//   uhc_sf_pose        a body's pose as the kernel keeps it: position and the rotation matrix of its quaternion
//   uhc_sf_world       w = xpos + R(xquat) v
//   uhc_sf_height      h = w.z - radius - floor_z
//   uhc_sf_below / uhc_sf_touches / uhc_sf_above   the three predicates: h < 0 (penetration), h <= 0 (skate, contact), h > 0 (float)
//   uhc_sf_slide       |w_xy[r + 1] - w_xy[r]|
#pragma once
#include <math.h>

#include "uhc_seq.h"  // uhc_nan

#if defined(__HIPCC__)
#define UHC_SF_HD __host__ __device__ __forceinline__
#else
#define UHC_SF_HD inline
#endif

#define UHC_SF_NMETRIC 4  // pen, skate, float, contact: the order of a d_row_out row
enum { UHC_SF_PEN = 0, UHC_SF_SKATE = 1, UHC_SF_FLOAT = 2, UHC_SF_CONTACT = 3 };
#define UHC_SF_POSE_DOUBLES 12  // a UhcSfPose as doubles: p[3], R[9]

struct UhcSfV3 {
    double x, y, z;
};

struct UhcSfPose {
    double p[3], R[9];
};

// position + the rotation of the quaternion (w, x, y, z), divided by its squared length: R = I + (2 / |q|^2) (...).  For a unit quaternion this is the
// usual matrix; a quaternion with small-integer components and |q|^2 a power of two -- (1, 1, 0, 0): a quarter turn -- gives entries that are exactly
// 0 and +-1, which is what lets a test put a vertex EXACTLY on the floor.  Below |q|^2 = 4 eps: the identity, as quaternion_matrix.
UHC_SF_HD UhcSfPose uhc_sf_pose(const double* pos3, const double* quat4) {
    UhcSfPose o;
    const double w = quat4[0], x = quat4[1], y = quat4[2], z = quat4[3];
    const double n = w * w + x * x + y * y + z * z;
    const double s = n < 4.0 * 2.220446049250313e-16 ? 0.0 : 2.0 / n;  // (selected, not branched)
    o.p[0] = pos3[0], o.p[1] = pos3[1], o.p[2] = pos3[2];
    o.R[0] = 1.0 - s * (y * y + z * z), o.R[1] = s * (x * y - z * w), o.R[2] = s * (x * z + y * w);
    o.R[3] = s * (x * y + z * w), o.R[4] = 1.0 - s * (x * x + z * z), o.R[5] = s * (y * z - x * w);
    o.R[6] = s * (x * z - y * w), o.R[7] = s * (y * z + x * w), o.R[8] = 1.0 - s * (x * x + y * y);
    return o;
}

// are the seven numbers of a pose finite?  (x - x is 0 for a finite x and NaN for an infinity or a NaN)
UHC_SF_HD bool uhc_sf_pose_finite(const double* pos3, const double* quat4) {
    const double a = (pos3[0] - pos3[0]) + (pos3[1] - pos3[1]) + (pos3[2] - pos3[2]);
    const double b = (quat4[0] - quat4[0]) + (quat4[1] - quat4[1]) + (quat4[2] - quat4[2]) + (quat4[3] - quat4[3]);
    return a + b == 0.0;
}

UHC_SF_HD UhcSfV3 uhc_sf_world(const UhcSfPose& P, double vx, double vy, double vz) {
    UhcSfV3 w;
    w.x = P.p[0] + ((P.R[0] * vx + P.R[1] * vy) + P.R[2] * vz);
    w.y = P.p[1] + ((P.R[3] * vx + P.R[4] * vy) + P.R[5] * vz);
    w.z = P.p[2] + ((P.R[6] * vx + P.R[7] * vy) + P.R[8] * vz);
    return w;
}

UHC_SF_HD double uhc_sf_height(const UhcSfV3& w, double radius, double floor_z) { return (w.z - radius) - floor_z; }
UHC_SF_HD bool uhc_sf_below(double h) { return h < 0.0; }     // strict: compute_penetration's `vert_z < 0`
UHC_SF_HD bool uhc_sf_touches(double h) { return h <= 0.0; }  // non-strict: compute_skate's `z <= floor_z`
UHC_SF_HD bool uhc_sf_above(double h) { return h > 0.0; }

UHC_SF_HD double uhc_sf_slide(const UhcSfV3& w0, const UhcSfV3& w1) {
    const double dx = w1.x - w0.x, dy = w1.y - w0.y;
    return sqrt(dx * dx + dy * dy);
}

// what one lane (or the host loop) carries over its vertices, and how two of them are joined (the wave's butterfly; the host never needs it)
struct UhcSfAcc {
    double pen_sum, skate_sum, h_min;
    int pen_n, skate_n, contact_n, above_n;
};

UHC_SF_HD UhcSfAcc uhc_sf_acc_zero() {
    UhcSfAcc a;
    a.pen_sum = a.skate_sum = 0.0;
    a.h_min = HUGE_VAL;
    a.pen_n = a.skate_n = a.contact_n = a.above_n = 0;
    return a;
}

// one vertex of row r: its own pose P0 and -- has_next -- its pose in row r + 1
UHC_SF_HD void uhc_sf_acc_vertex(UhcSfAcc& a, const UhcSfPose& P0, const UhcSfPose& P1, bool has_next, double vx, double vy, double vz, double radius, double floor_z) {
    const UhcSfV3 w0 = uhc_sf_world(P0, vx, vy, vz);
    const double h0 = uhc_sf_height(w0, radius, floor_z);
    if (uhc_sf_below(h0)) a.pen_sum += h0, a.pen_n++;
    if (uhc_sf_touches(h0)) a.contact_n++;
    if (uhc_sf_above(h0)) a.above_n++;
    a.h_min = h0 < a.h_min ? h0 : a.h_min;
    if (has_next) {
        const UhcSfV3 w1 = uhc_sf_world(P1, vx, vy, vz);
        if (uhc_sf_touches(h0) && uhc_sf_touches(uhc_sf_height(w1, radius, floor_z))) a.skate_sum += uhc_sf_slide(w0, w1), a.skate_n++;
    }
}

// the row's four values from the sums over its n_vert vertices, in mm; out[UHC_SF_SKATE] is written only where row r + 1 exists
UHC_SF_HD void uhc_sf_finish(const UhcSfAcc& a, int n_vert, bool has_next, double* out) {
    out[UHC_SF_PEN] = a.pen_n > 0 ? -(a.pen_sum / a.pen_n) * 1000.0 : 0.0;
    if (has_next) out[UHC_SF_SKATE] = a.skate_n > 0 ? a.skate_sum / a.skate_n * 1000.0 : 0.0;
    out[UHC_SF_FLOAT] = a.above_n == n_vert ? a.h_min * 1000.0 : 0.0;
    out[UHC_SF_CONTACT] = (double)a.contact_n;
}

// The row as every path stores it -- the kernels (uhc_surface.hip, uhc_smpl_mesh.hip) and the host loop below: uhc_sf_finish's values where the row's own poses
// are finite (row_ok), with the skate NaN where the next row's are not (next_ok); NaN throughout for a bad row.  The skate slot is left alone without a next row.
UHC_SF_HD void uhc_sf_store_row(double* out, const UhcSfAcc& acc, int n_vert, bool has_next, bool row_ok, bool next_ok) {
    if (row_ok) {
        uhc_sf_finish(acc, n_vert, has_next, out);
        if (has_next && !next_ok) out[UHC_SF_SKATE] = uhc_nan();
    } else {
        out[UHC_SF_PEN] = out[UHC_SF_FLOAT] = out[UHC_SF_CONTACT] = uhc_nan();
        if (has_next) out[UHC_SF_SKATE] = uhc_nan();
    }
}

// One row, the sums over the vertices as a plain loop in vertex order.  pos0 / quat0: [n_body][3] / [n_body][4] of row r; pos1 / quat1: of row r + 1 (read only
// when has_next); vert [n_vert][3] in the body frame, vert_body [n_vert] (0 .. n_body - 1), vert_radius [n_vert] or NULL.  A non-finite pose number in row r:
// the four values are NaN; in row r + 1: the skate is.  Returns 1 when row r is such a row (the caller's `bad` count), else 0.
inline int uhc_sf_row_serial(int n_body, int n_vert, const int* vert_body, const double* vert_radius, const double* vert, const double* pos0, const double* quat0,
                             const double* pos1, const double* quat1, bool has_next, double floor_z, double* out) {
    bool ok0 = true, ok1 = true;
    for (int b = 0; b < n_body; b++) {
        ok0 = ok0 && uhc_sf_pose_finite(pos0 + 3 * b, quat0 + 4 * b);
        if (has_next) ok1 = ok1 && uhc_sf_pose_finite(pos1 + 3 * b, quat1 + 4 * b);
    }
    UhcSfAcc a = uhc_sf_acc_zero();
    for (int v = 0; v < n_vert; v++) {
        const int b = vert_body[v];
        const UhcSfPose P0 = uhc_sf_pose(pos0 + 3 * b, quat0 + 4 * b);
        const UhcSfPose P1 = has_next ? uhc_sf_pose(pos1 + 3 * b, quat1 + 4 * b) : P0;
        uhc_sf_acc_vertex(a, P0, P1, has_next, vert[3 * v], vert[3 * v + 1], vert[3 * v + 2], vert_radius ? vert_radius[v] : 0.0, floor_z);
    }
    uhc_sf_store_row(out, a, n_vert, has_next, ok0, ok1);
    return ok0 ? 0 : 1;
}
