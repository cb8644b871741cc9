// Host build of uhc_amd/csrc/uhc_surface_math.h for tests/test_surface_metrics_cpu.py: the header's per-vertex arithmetic, the sums over the vertices and the
// means over the rows as plain loops -- what uhc_surface.hip computes with the vertices dealt to the lanes.  No HIP header, no hipcc.
#include "uhc_surface_math.h"

#define PROBE_API extern "C" __attribute__((visibility("default")))

// One sequence of T rows.  pos [T][n_body][3], quat [T][n_body][4]; vert [n_vert][3] (the sequence's model), vert_body [n_vert], vert_radius [n_vert] or NULL.
// row_out [T][4]: written as uhc_surface_metrics writes it (the skate of the last row is left alone); means [4]: over T, T - 1, T, T rows, NaN over none.
// Returns the number of rows with a non-finite pose.
PROBE_API int uhc_surface_probe_seq(int n_body, int n_vert, const int* vert_body, const double* vert_radius, const double* vert, const double* pos,
                                    const double* quat, int T, double floor_z, double* row_out, double* means) {
    int bad = 0;
    for (int r = 0; r < T; r++) {
        const bool has_next = r + 1 < T;
        const double* p0 = pos + (long)r * n_body * 3;
        const double* q0 = quat + (long)r * n_body * 4;
        bad += uhc_sf_row_serial(n_body, n_vert, vert_body, vert_radius, vert, p0, q0, has_next ? p0 + n_body * 3 : p0, has_next ? q0 + n_body * 4 : q0, has_next,
                                 floor_z, row_out + (long)r * UHC_SF_NMETRIC);
    }
    for (int k = 0; k < UHC_SF_NMETRIC; k++) {
        const int n = T - (k == UHC_SF_SKATE ? 1 : 0);
        double s = 0.0;
        for (int r = 0; r < n; r++) s += row_out[(long)r * UHC_SF_NMETRIC + k];
        means[k] = n > 0 ? s / n : NAN;
    }
    return bad;
}

// the finished row as the kernels and the loop above store it (uhc_sf_store_row); acc7: pen_sum, skate_sum, h_min, pen_n, skate_n, contact_n, above_n
PROBE_API void uhc_surface_probe_store_row(const double* acc7, int n_vert, int has_next, int row_ok, int next_ok, double* out) {
    UhcSfAcc a;
    a.pen_sum = acc7[0], a.skate_sum = acc7[1], a.h_min = acc7[2];
    a.pen_n = (int)acc7[3], a.skate_n = (int)acc7[4], a.contact_n = (int)acc7[5], a.above_n = (int)acc7[6];
    uhc_sf_store_row(out, a, n_vert, has_next != 0, row_ok != 0, next_ok != 0);
}

// one vertex: world position (out[0:3]), height (out[3]) and the three predicates (out[4:7] as 0 / 1)
PROBE_API void uhc_surface_probe_vertex(const double* pos3, const double* quat4, const double* v3, double radius, double floor_z, double* out) {
    const UhcSfPose P = uhc_sf_pose(pos3, quat4);
    const UhcSfV3 w = uhc_sf_world(P, v3[0], v3[1], v3[2]);
    const double h = uhc_sf_height(w, radius, floor_z);
    out[0] = w.x, out[1] = w.y, out[2] = w.z, out[3] = h;
    out[4] = uhc_sf_below(h), out[5] = uhc_sf_touches(h), out[6] = uhc_sf_above(h);
}
