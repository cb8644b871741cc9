// Contact quality of a motion on the device: uhc_surface_create / _free / _metrics (include/uhc_amd.h).
//
// Penetration, skate, float and contact count of a sequence of body poses (reference: compute_penetration / compute_skate, uhc/smpllib/smpl_eval.py:125-149,
// there on SMPL surface vertices; here on the convex-hull vertices every compiled model carries in the body frame).  The poses are read where they lie:
// a pose record (uhc_eval.hip: uhc_eval_record_pose appends xpos / xquat of bodies 1 .. 24 beside uhc_eval_record's rows) or the clip bank's frame records.
//
//   uhc_surface_rows_kernel      one wave per (sequence, row), four waves per workgroup.  Lanes 0 .. n_body - 1 load the row's and the next row's body poses,
//                                turn the quaternions into matrices and put both into the wave's slice of LDS (24 doubles a body); the vertices are dealt to
//                                the lanes with stride 64, each lane reads its vertex's two poses from LDS and keeps partial sums in vertex order; the wave
//                                finishes with xor butterflies (32, 16, .., 1: every lane ends with the same bits, in an order fixed by the lane numbers alone).
//                                The arithmetic of a vertex is uhc_surface_math.h, which the CPU test compiles for the host.
//   uhc_surface_means_kernel     one thread per (sequence, metric): the mean over the sequence's rows in row order.
// No floating-point atomics; the one counter that is added to (d_bad) is an integer.  No index or counter, whatever it holds, sends a read or a write outside
// the arrays (uhc_seq.h: row counts are clamped to 0 .. row_cap, a sequence whose rows leave 0 .. n_rows_total is skipped, a model index outside the range
// reads as 0).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uhc_amd.h"
#include "uhc_api_check.h"

#include <vector>

#pragma clang fp contract(off)
#include "uhc_seq.h"
#include "uhc_surface_math.h"

#define SF_WAVES 4  // waves per workgroup

struct UhcSurface {
    int n_body, n_vert, n_models;
    int* d_vert_body;       // [n_vert]
    double* d_vert_radius;  // [n_vert]
    double* d_vert;         // [n_models][n_vert][3]
};

struct SurfaceArgs {
    int n_body, n_vert, n_models, n_seq, row_cap;
    long long n_rows_total, pos_stride, quat_stride;
    double floor_z;
    const int* vert_body;
    const double *vert_radius, *vert;
    const long long* seq_start;
    const int *seq_rows, *seq_model;
    const double *pos, *quat;
    double *row_out, *seq_means;
    int* bad;
};

__device__ __forceinline__ UhcSfPose sf_lds_pose(const double* p) {
    UhcSfPose P;
#pragma unroll
    for (int k = 0; k < 3; k++) P.p[k] = p[k];
#pragma unroll
    for (int k = 0; k < 9; k++) P.R[k] = p[3 + k];
    return P;
}

__global__ void __launch_bounds__(64 * SF_WAVES) uhc_surface_rows_kernel(const SurfaceArgs A) {
    extern __shared__ __attribute__((aligned(16))) double sf_lds[];  // [SF_WAVES][n_body][2][12]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long R = (long long)blockIdx.x * SF_WAVES + wave;
    // (no wave leaves before the barrier: one without a row loads nothing and stores nothing)
    const bool in_grid = R < (long long)A.n_seq * A.row_cap;
    const int s = in_grid ? (int)(R / A.row_cap) : 0, r = in_grid ? (int)(R % A.row_cap) : 0;
    const int T = in_grid ? uhc_seq_rows(A.seq_rows[s], A.row_cap) : 0;
    const long long g0 = in_grid ? uhc_seq_start(A.seq_start[s], T, A.n_rows_total) : -1;
    const bool valid = in_grid && r < T && g0 >= 0;
    const bool has_next = valid && r + 1 < T;
    const long long g = valid ? g0 + r : 0;  // (g + 1 < g0 + T <= n_rows_total where has_next)
    const int model = uhc_seq_model(valid ? A.seq_model : nullptr, s, A.n_models);  // (a wave without a row reads no table)

    double* mine = sf_lds + (size_t)wave * A.n_body * 2 * UHC_SF_POSE_DOUBLES;
    bool ok0 = true, ok1 = true;
    if (valid && lane < A.n_body) {
        const double* p = A.pos + g * A.pos_stride + 3 * lane;
        const double* q = A.quat + g * A.quat_stride + 4 * lane;
        const double p0[3] = {p[0], p[1], p[2]}, q0[4] = {q[0], q[1], q[2], q[3]};
        double p1[3] = {p0[0], p0[1], p0[2]}, q1[4] = {q0[0], q0[1], q0[2], q0[3]};
        if (has_next) {
            const double* pn = p + A.pos_stride;
            const double* qn = q + A.quat_stride;
            p1[0] = pn[0], p1[1] = pn[1], p1[2] = pn[2];
            q1[0] = qn[0], q1[1] = qn[1], q1[2] = qn[2], q1[3] = qn[3];
        }
        ok0 = uhc_sf_pose_finite(p0, q0), ok1 = uhc_sf_pose_finite(p1, q1);
        const UhcSfPose P0 = uhc_sf_pose(p0, q0), P1 = uhc_sf_pose(p1, q1);
        double* o = mine + (size_t)lane * 2 * UHC_SF_POSE_DOUBLES;
#pragma unroll
        for (int k = 0; k < 3; k++) o[k] = P0.p[k], o[UHC_SF_POSE_DOUBLES + k] = P1.p[k];
#pragma unroll
        for (int k = 0; k < 9; k++) o[3 + k] = P0.R[k], o[UHC_SF_POSE_DOUBLES + 3 + k] = P1.R[k];
    }
    __syncthreads();
    const bool row_ok = __all(ok0), next_ok = __all(ok1);

    UhcSfAcc a = uhc_sf_acc_zero();
    if (valid) {
        const double* vert = A.vert + (size_t)model * A.n_vert * 3;
        for (int v = lane; v < A.n_vert; v += 64) {
            int b = A.vert_body[v];
            b = b >= 0 && b < A.n_body ? b : 0;  // (uhc_surface_create refused anything else)
            const double* pb = mine + (size_t)b * 2 * UHC_SF_POSE_DOUBLES;
            const UhcSfPose P0 = sf_lds_pose(pb), P1 = sf_lds_pose(pb + UHC_SF_POSE_DOUBLES);
            uhc_sf_acc_vertex(a, P0, P1, has_next, vert[3 * v], vert[3 * v + 1], vert[3 * v + 2], A.vert_radius[v], A.floor_z);
        }
    }
    // (every lane of every wave takes part in the butterflies)
    UhcSfAcc w;
    w.pen_sum = uhc_xor_sum<32>(a.pen_sum), w.skate_sum = uhc_xor_sum<32>(a.skate_sum), w.h_min = uhc_xor_min<32>(a.h_min);
    w.pen_n = uhc_xor_sum<32>(a.pen_n), w.skate_n = uhc_xor_sum<32>(a.skate_n), w.contact_n = uhc_xor_sum<32>(a.contact_n), w.above_n = uhc_xor_sum<32>(a.above_n);

    if (valid && lane == 0) {
        uhc_sf_store_row(A.row_out + (size_t)g * UHC_SF_NMETRIC, w, A.n_vert, has_next, row_ok, next_ok);
        if (!row_ok) atomicAdd(A.bad, 1);  // one count per bad row: by the wave that owns it
    }
}

__global__ void __launch_bounds__(256) uhc_surface_means_kernel(const SurfaceArgs A) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= A.n_seq * UHC_SF_NMETRIC) return;
    const int s = idx / UHC_SF_NMETRIC, k = idx % UHC_SF_NMETRIC;
    const int T = uhc_seq_rows(A.seq_rows[s], A.row_cap);
    const long long g0 = uhc_seq_start(A.seq_start[s], T, A.n_rows_total);
    if (g0 < 0) {  // the sequence is skipped: nothing of it is read or written
        if (k == 0) atomicAdd(A.bad, 1);
        return;
    }
    A.seq_means[idx] = uhc_seq_mean(A.row_out, UHC_SF_NMETRIC, k, g0, T - (k == UHC_SF_SKATE ? 1 : 0));  // (the skate: over the T - 1 pairs of rows)
}

// ------------------------------------------------------------------ C-ABI (include/uhc_amd.h)
extern "C" int32_t uhc_surface_create(int32_t n_body, int32_t n_vert, int32_t n_models, const int32_t* h_vert_body, const double* h_vert_radius,
                                      const double* h_vert, UhcSurface** out) {
    // every check comes before the first HIP call
    REFUSE("uhc_surface_create", !out, "out is NULL");
    *out = nullptr;
    REFUSE("uhc_surface_create", n_body < 1 || n_body > 64, "n_body must be 1 .. 64 (one lane per body)");
    REFUSE("uhc_surface_create", n_vert < 1 || n_vert > 65535, "n_vert must be 1 .. 65535");
    REFUSE("uhc_surface_create", n_models < 1, "n_models < 1");
    REFUSE("uhc_surface_create", (long long)n_models * n_vert > 0x7fffffffLL / 3, "n_models x n_vert is beyond the tables' index range");
    REFUSE("uhc_surface_create", !h_vert_body, "h_vert_body is NULL");
    REFUSE("uhc_surface_create", !h_vert, "h_vert is NULL");
    for (int v = 0; v < n_vert; v++) {
        REFUSE("uhc_surface_create", h_vert_body[v] < 0 || h_vert_body[v] >= n_body, "h_vert_body holds a body outside 0 .. n_body - 1");
        REFUSE("uhc_surface_create", h_vert_radius && !(std::isfinite(h_vert_radius[v]) && h_vert_radius[v] >= 0.0), "h_vert_radius holds a negative or non-finite radius");
    }
    const size_t n3 = (size_t)n_models * n_vert * 3;
    REFUSE("uhc_surface_create", !uhc_all_finite(h_vert, n3), "h_vert holds a non-finite coordinate");
    std::vector<double> radius(n_vert, 0.0);
    if (h_vert_radius) radius.assign(h_vert_radius, h_vert_radius + n_vert);
    UhcSurface* S = new UhcSurface();
    *S = UhcSurface{};
    S->n_body = n_body, S->n_vert = n_vert, S->n_models = n_models;
    hipError_t e = uhc_upload(&S->d_vert_body, h_vert_body, n_vert);
    if (e == hipSuccess) e = uhc_upload(&S->d_vert_radius, radius.data(), n_vert);
    if (e == hipSuccess) e = uhc_upload(&S->d_vert, h_vert, n3);
    if (e != hipSuccess) {
        uhc_surface_free(S);
        return uhc_internal_set_error((std::string("uhc_surface_create: ") + hipGetErrorString(e)).c_str());
    }
    *out = S;
    return 0;
}

extern "C" void uhc_surface_free(UhcSurface* S) {
    if (!S) return;
    void* all[] = {S->d_vert_body, S->d_vert_radius, S->d_vert};
    for (void* p : all)
        if (p) (void)hipFree(p);
    delete S;
}

extern "C" int32_t uhc_surface_metrics(void* stream, const UhcSurface* surf, int32_t n_seq, const int64_t* d_seq_start, const int32_t* d_seq_rows, int32_t row_cap,
                                       const int32_t* d_seq_model, const double* d_pos, int64_t pos_stride, const double* d_quat, int64_t quat_stride,
                                       int64_t n_rows_total, double floor_z, double* d_row_out, double* d_seq_means, int32_t* d_bad, int32_t* h_bad) {
    REFUSE("uhc_surface_metrics", !surf, "surf is NULL");
    REFUSE("uhc_surface_metrics", n_seq < 0, "n_seq < 0");
    REFUSE("uhc_surface_metrics", row_cap <= 0, "row_cap <= 0");
    REFUSE("uhc_surface_metrics", n_rows_total < 0, "n_rows_total < 0");
    REFUSE("uhc_surface_metrics", pos_stride < 3, "pos_stride is below 3 n_body (rows would overlap)");
    REFUSE("uhc_surface_metrics", quat_stride < 4, "quat_stride is below 4 n_body (rows would overlap)");
    REFUSE("uhc_surface_metrics", pos_stride > (1LL << 31) || quat_stride > (1LL << 31) || n_rows_total > (1LL << 31), "pos_stride, quat_stride or n_rows_total is beyond 2^31");
    REFUSE("uhc_surface_metrics", !std::isfinite(floor_z), "floor_z is not finite");
    REFUSE("uhc_surface_metrics", !d_seq_start, "d_seq_start is NULL");
    REFUSE("uhc_surface_metrics", !d_seq_rows, "d_seq_rows is NULL");
    REFUSE("uhc_surface_metrics", !d_pos, "d_pos is NULL");
    REFUSE("uhc_surface_metrics", !d_quat, "d_quat is NULL");
    REFUSE("uhc_surface_metrics", !d_row_out, "d_row_out is NULL");
    REFUSE("uhc_surface_metrics", !d_seq_means, "d_seq_means is NULL");
    REFUSE("uhc_surface_metrics", !d_bad, "d_bad is NULL");
    const long long blocks = ((long long)n_seq * row_cap + SF_WAVES - 1) / SF_WAVES;
    REFUSE("uhc_surface_metrics", !uhc_launch_fits(blocks) || !uhc_launch_fits((long long)n_seq * UHC_SF_NMETRIC), "n_seq x row_cap is beyond one launch");
    if (n_seq == 0) {
        if (h_bad) *h_bad = 0;
        return 0;
    }
    // (the two checks that read the handle: behind the empty return, still before the first HIP call)
    REFUSE("uhc_surface_metrics", pos_stride < 3LL * surf->n_body, "pos_stride is below 3 n_body (rows would overlap)");
    REFUSE("uhc_surface_metrics", quat_stride < 4LL * surf->n_body, "quat_stride is below 4 n_body (rows would overlap)");
    SurfaceArgs A = {};
    A.n_body = surf->n_body, A.n_vert = surf->n_vert, A.n_models = surf->n_models, A.n_seq = n_seq, A.row_cap = row_cap;
    A.n_rows_total = n_rows_total, A.pos_stride = pos_stride, A.quat_stride = quat_stride, A.floor_z = floor_z;
    A.vert_body = surf->d_vert_body, A.vert_radius = surf->d_vert_radius, A.vert = surf->d_vert;
    A.seq_start = (const long long*)d_seq_start, A.seq_rows = d_seq_rows, A.seq_model = d_seq_model, A.pos = d_pos, A.quat = d_quat;
    A.row_out = d_row_out, A.seq_means = d_seq_means, A.bad = d_bad;
    hipStream_t s = (hipStream_t)stream;
    HIP_OK(hipMemsetAsync(d_bad, 0, sizeof(int32_t), s));
    const size_t lds = sizeof(double) * SF_WAVES * surf->n_body * 2 * UHC_SF_POSE_DOUBLES;  // (at most 48 KiB: n_body <= 64)
    hipLaunchKernelGGL(uhc_surface_rows_kernel, dim3((unsigned)blocks), dim3(64 * SF_WAVES), lds, s, A);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(uhc_surface_means_kernel, dim3((unsigned)((n_seq * UHC_SF_NMETRIC + 255) / 256)), dim3(256), 0, s, A);
    HIP_OK(hipGetLastError());
    return uhc_return_bad(h_bad, d_bad, s);
}
