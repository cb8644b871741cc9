// The SMPL body mesh on the device: uhc_smpl_mesh_create / _free, uhc_smpl_mesh (include/uhc_amd.h).
//
// Vertices, joints and the contact quality of posed SMPL bodies (reference: SMPL_Parser.get_joints_verts, uhc/smpllib/smpl_parser.py:335-360 -- smplx's lbs --
// and compute_penetration / compute_skate on its vertices, uhc/smpllib/smpl_eval.py:113-149), float64.  The poses are read where uhc_qpos_smpl left them.
//
//   uhc_smpl_shape_kernel    one thread per (sequence, vertex): v_shaped = v_template + shapedirs beta.  Thread 0 of a sequence counts it when it is skipped.
//   uhc_smpl_joints_kernel   one workgroup per (sequence, joint): J = J_regressor v_shaped, strided partial sums and a tree in LDS (a fixed order).
//   uhc_smpl_mesh_kernel     one wave per row tile (16 rows of one sequence, 15 of them its own), four waves per workgroup.  Lanes 0 .. 15 turn their row's 24
//                            rotation vectors into matrices in the wave's slice of LDS; every lane takes its 52 A operands (the feature R - I) from there; lanes
//                            0 .. 15 then run the chain in place, which leaves the 24 transforms A_j of the 16 rows.  The wave walks the vertex tiles: 3 x 52
//                            v_mfma_f64_16x16x4_f64 give the pose offsets of 16 vertices x 16 rows, lane l holding x, y, z of vertex l & 15 for the rows
//                            (l >> 4) + 4 i; it skins them from the (joint, weight) list of its vertex, stores them, and keeps the row's partial sums.  The
//                            skate's next row comes from the lane 16 further on (__shfl).  The four waves of a workgroup walk the same tiles between the same
//                            barriers, so a load of the packed posedirs by one of them is in the cache for the other three: 64 rows (60 owned) per load.
//   uhc_smpl_means_kernel    one thread per (sequence, metric): the mean over the sequence's rows in row order.
// No floating-point atomics: a row's sums are per-lane partial sums in vertex-tile order and xor butterflies over the 16 lanes of its group.  No index, whatever
// it holds, sends a read or a write outside the arrays (uhc_seq.h: row counts clamped, a sequence outside the rows skipped, a model index outside the range
// reads as 0).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uhc_amd.h"
#include "uhc_api_check.h"

#include <vector>

#pragma clang fp contract(off)
#include "uhc_seq.h"
#include "uhc_smpl_mesh_math.h"
#include "uhc_surface_math.h"

#define SM_WAVES 4  // waves (row tiles) per workgroup
#define SM_LDS_BYTES (sizeof(double) * SM_WAVES * UHC_SM_G_WAVE)

struct UhcSmplMesh {
    int n_vert, n_vtiles, n_models, nw;
    int parents[UHC_SM_NJ];
    double *d_v_template, *d_shapedirs, *d_jreg;  // [n_models][n_vert][3], [..][n_vert][3][10], [..][24][n_vert]
    double* d_posedirs;                           // [n_models][sm_b_doubles(n_vert)]: packed (sm_b_index)
    int* d_wj;                                    // [n_models][16 n_vtiles][nw]: the joints of a vertex's non-zero skin weights, ascending; padding (0, 0.0)
    double* d_ww;
    // what a call keeps between its kernels; it grows with the call (a handle serves one stream at a time)
    double *d_v_shaped, *d_J, *d_rows;  // [n_seq][16 n_vtiles][3], [n_seq][24][3]; [n_rows_total][4] when the caller wants means without rows
    size_t cap_seq, cap_rows;
    bool lds_set;
};

struct MeshArgs {
    int n_vert, n_vtiles, n_models, nw, n_seq, row_cap, tiles_per_seq, want_vert_loop, want_metrics;
    int parents[UHC_SM_NJ];
    long long n_rows_total, pose_stride, trans_stride;
    double floor_z;
    const double *v_template, *shapedirs, *jreg, *posedirs, *ww;
    const int* wj;
    const long long* seq_start;
    const int *seq_rows, *seq_model;
    const double *betas, *pose, *trans;
    double *v_shaped, *J;
    double *vert, *joints, *row_out, *seq_means, *zmin;
    int* bad;
};

// sequence s as uhc_seq.h reads it: its rows, its first global row (-1: skipped), its model
__device__ __forceinline__ int sm_rows_of(const MeshArgs& A, int s) { return uhc_seq_rows(A.seq_rows[s], A.row_cap); }
__device__ __forceinline__ long long sm_start_of(const MeshArgs& A, int s, int T) { return uhc_seq_start(A.seq_start[s], T, A.n_rows_total); }
__device__ __forceinline__ int sm_model_of(const MeshArgs& A, int s) { return uhc_seq_model(A.seq_model, s, A.n_models); }

__global__ void __launch_bounds__(256) uhc_smpl_shape_kernel(const MeshArgs A) {
    const int vpad = UHC_SM_TILE * A.n_vtiles, per_seq = (vpad + 255) / 256;  // (the sequence rides in blockIdx.x: no 65 535 limit of a grid's y)
    const int s = blockIdx.x / per_seq, v = (blockIdx.x % per_seq) * 256 + threadIdx.x;
    if (v == 0 && sm_start_of(A, s, sm_rows_of(A, s)) < 0) atomicAdd(A.bad, 1);  // one count per skipped sequence
    if (v >= vpad) return;
    double* out = A.v_shaped + ((size_t)s * vpad + v) * 3;
    if (v >= A.n_vert) {  // the padding of the last vertex tile
        out[0] = out[1] = out[2] = 0.0;
        return;
    }
    const int m = sm_model_of(A, s);
    const double* beta = A.betas + (size_t)s * UHC_SM_NBETA;
    const double* vt = A.v_template + ((size_t)m * A.n_vert + v) * 3;
    const double* sd = A.shapedirs + ((size_t)m * A.n_vert + v) * 3 * UHC_SM_NBETA;
    for (int c = 0; c < 3; c++) {
        double d = 0.0;
        for (int b = 0; b < UHC_SM_NBETA; b++) d += sd[c * UHC_SM_NBETA + b] * beta[b];
        out[c] = vt[c] + d;
    }
}

__global__ void __launch_bounds__(256) uhc_smpl_joints_kernel(const MeshArgs A) {
    __shared__ double part[3][256];
    const int j = blockIdx.x % UHC_SM_NJ, s = blockIdx.x / UHC_SM_NJ, t = threadIdx.x, vpad = UHC_SM_TILE * A.n_vtiles;
    const int m = sm_model_of(A, s);
    const double* reg = A.jreg + ((size_t)m * UHC_SM_NJ + j) * A.n_vert;
    const double* vs = A.v_shaped + (size_t)s * vpad * 3;
    double a[3] = {0.0, 0.0, 0.0};
    for (int v = t; v < A.n_vert; v += 256)
        for (int c = 0; c < 3; c++) a[c] += reg[v] * vs[3 * v + c];
    for (int c = 0; c < 3; c++) part[c][t] = a[c];
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h)
            for (int c = 0; c < 3; c++) part[c][t] += part[c][t + h];
        __syncthreads();
    }
    if (t < 3) A.J[((size_t)s * UHC_SM_NJ + j) * 3 + t] = part[t][0];
}

typedef double sm_acc __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(64 * SM_WAVES) uhc_smpl_mesh_kernel(const MeshArgs A) {
    extern __shared__ __attribute__((aligned(16))) double sm_lds[];  // [SM_WAVES][UHC_SM_G_WAVE]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane >> 4;
    const double nan = uhc_nan();
    // (no wave leaves before the last barrier: one without rows loads nothing and stores nothing)
    const long long R = (long long)blockIdx.x * SM_WAVES + wave;
    const bool in_grid = R < (long long)A.n_seq * A.tiles_per_seq;
    const int s = in_grid ? (int)(R / A.tiles_per_seq) : 0, r0 = in_grid ? sm_tile_row0((int)(R % A.tiles_per_seq)) : 0;
    const int T = in_grid ? sm_rows_of(A, s) : 0;
    const long long g0 = in_grid ? sm_start_of(A, s, T) : -1;
    const bool active = in_grid && g0 >= 0 && r0 < T;  // (wave-uniform)
    const int model = active ? sm_model_of(A, s) : 0;
    const int vpad = UHC_SM_TILE * A.n_vtiles;
    double* G = sm_lds + (size_t)wave * UHC_SM_G_WAVE;

    // ---- lanes 0 .. 15, one row each: the 24 local rotations into LDS.  A row beyond the sequence's end is the zero pose (R = I, feature 0) and is never read.
    const bool row_exists = active && lane < UHC_SM_TILE && r0 + lane < T;
    const long long g_mine = row_exists ? g0 + r0 + lane : 0;  // (< g0 + T <= n_rows_total)
    bool ok = true;
    double tr[3] = {0.0, 0.0, 0.0};
    if (active && lane < UHC_SM_TILE) {
        const double* pp = A.pose + g_mine * A.pose_stride;
        for (int j = 0; j < UHC_SM_NJ; j++) {
            double r3[3] = {0.0, 0.0, 0.0}, Rl[9];
            if (row_exists) r3[0] = pp[3 * j], r3[1] = pp[3 * j + 1], r3[2] = pp[3 * j + 2];
            ok = ok && sm_finite3(r3);
            sm_rodrigues(r3, Rl);
#pragma unroll
            for (int e = 0; e < 9; e++) G[sm_g_index(j, e, lane)] = Rl[e];
        }
        if (row_exists) {
            const double* tp = A.trans + g_mine * A.trans_stride;
            tr[0] = tp[0], tr[1] = tp[1], tr[2] = tp[2];
        }
        ok = ok && sm_finite3(tr);
    }
    __syncthreads();

    // ---- every lane: its A operands, feature[row lane & 15][k = 4 p + (lane >> 4)] = R_j[e] - I[e]
    double a[UHC_SM_KSTEPS];
#pragma unroll
    for (int p = 0; p < UHC_SM_KSTEPS; p++) {
        const int k = sm_a_k(p, lane);
        a[p] = 0.0;
        if (active && A.want_vert_loop && k < UHC_SM_NFEAT) a[p] = G[sm_g_index(sm_feat_joint(k), sm_feat_elem(k), sm_a_row(lane))] - sm_feat_identity(sm_feat_elem(k));
    }
    __syncthreads();

    // ---- lanes 0 .. 15: the chain, in place (parent[j] < j: a parent's slot already holds its global transform), then the shift to rest-pose points
    const bool row_owned = row_exists && lane < UHC_SM_OWNED;
    if (active && lane < UHC_SM_TILE) {
        const double* J = A.J + (size_t)s * UHC_SM_NJ * 3;
        for (int j = 0; j < UHC_SM_NJ; j++) {
            int p = A.parents[j];
            p = p >= 0 && p < j ? p : -1;  // (uhc_smpl_mesh_create refused anything else)
            double Rl[9], OR[9], Ot[3];
#pragma unroll
            for (int e = 0; e < 9; e++) Rl[e] = G[sm_g_index(j, e, lane)];
            if (p < 0) {
#pragma unroll
                for (int e = 0; e < 9; e++) OR[e] = Rl[e];
                Ot[0] = J[3 * j], Ot[1] = J[3 * j + 1], Ot[2] = J[3 * j + 2];
            } else {
                double PR[9], Pt[3];
#pragma unroll
                for (int e = 0; e < 9; e++) PR[e] = G[sm_g_index(p, e, lane)];
#pragma unroll
                for (int e = 0; e < 3; e++) Pt[e] = G[sm_g_index(p, 9 + e, lane)];
                const double d[3] = {J[3 * j] - J[3 * p], J[3 * j + 1] - J[3 * p + 1], J[3 * j + 2] - J[3 * p + 2]};
                sm_compose(PR, Pt, Rl, d, OR, Ot);
            }
#pragma unroll
            for (int e = 0; e < 9; e++) G[sm_g_index(j, e, lane)] = OR[e];
#pragma unroll
            for (int e = 0; e < 3; e++) G[sm_g_index(j, 9 + e, lane)] = Ot[e];
            if (row_owned && A.joints) {
                double* o = A.joints + ((size_t)g_mine * UHC_SM_NJ + j) * 3;
#pragma unroll
                for (int e = 0; e < 3; e++) o[e] = ok ? Ot[e] + tr[e] : nan;
            }
        }
        for (int j = 0; j < UHC_SM_NJ; j++) {
            double Rg[9], t[3], ts[3];
#pragma unroll
            for (int e = 0; e < 9; e++) Rg[e] = G[sm_g_index(j, e, lane)];
#pragma unroll
            for (int e = 0; e < 3; e++) t[e] = G[sm_g_index(j, 9 + e, lane)];
            sm_rest_shift(Rg, t, J + 3 * j, ts);
#pragma unroll
            for (int e = 0; e < 3; e++) G[sm_g_index(j, 9 + e, lane)] = ts[e];
        }
        if (row_owned && !ok) atomicAdd(A.bad, 1);  // one count per bad row: by the lane that owns it
    }
    __syncthreads();

    // ---- what a lane needs of its four rows (register i: row (lane >> 4) + 4 i of the tile)
    bool owned[4], has_next[4], row_ok[4], next_ok[4];
    double trans[4][3];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int lr = sm_cd_row(lane, i);
        owned[i] = active && lr < UHC_SM_OWNED && r0 + lr < T;
        has_next[i] = owned[i] && r0 + lr + 1 < T;
        row_ok[i] = __shfl((int)ok, lr) != 0;
        next_ok[i] = __shfl((int)ok, (lr + 1) & 15) != 0;
#pragma unroll
        for (int c = 0; c < 3; c++) trans[i][c] = __shfl(tr[c], lr);
    }

    double pen_sum[4], skate_sum[4], z_min[4];
    int pen_n[4], skate_n[4], contact_n[4], above_n[4];
#pragma unroll
    for (int i = 0; i < 4; i++) pen_sum[i] = skate_sum[i] = 0.0, z_min[i] = HUGE_VAL, pen_n[i] = skate_n[i] = contact_n[i] = above_n[i] = 0;

    if (A.want_vert_loop) {
        const double* Bm = A.posedirs + (size_t)model * sm_b_doubles(A.n_vert) + lane;
        const double* vs_s = A.v_shaped + (size_t)s * vpad * 3;
        for (int vt = 0; vt < A.n_vtiles; vt++) {
            if (active) {
                const double* B = Bm + sm_b_index(vt, 0, 0, 0);
                sm_acc acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = acc0, acc2 = acc0;
#pragma unroll
                for (int p = 0; p < UHC_SM_KSTEPS; p++) {  // (lane l reads B[64 p + l]: k = 4 p + (l >> 4), vertex l & 15 -- sm_b_index)
                    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[p], B[64 * p], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[p], B[UHC_SM_KPAD * UHC_SM_TILE + 64 * p], acc1, 0, 0, 0);
                    acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[p], B[2 * UHC_SM_KPAD * UHC_SM_TILE + 64 * p], acc2, 0, 0, 0);
                }
                const int v = UHC_SM_TILE * vt + sm_cd_vert(lane);  // (< vpad: the tables are padded)
                const bool v_real = v < A.n_vert;
                const double vs[3] = {vs_s[3 * v], vs_s[3 * v + 1], vs_s[3 * v + 2]};
                const int* wj = A.wj + ((size_t)model * vpad + v) * A.nw;
                const double* ww = A.ww + ((size_t)model * vpad + v) * A.nw;
                double wx[4], wy[4];
                bool touch[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int lr = sm_cd_row(lane, i);
                    const double vp[3] = {vs[0] + acc0[i], vs[1] + acc1[i], vs[2] + acc2[i]};
                    double Tm[UHC_SM_XF];
#pragma unroll
                    for (int c = 0; c < UHC_SM_XF; c++) Tm[c] = 0.0;
                    for (int q = 0; q < A.nw; q++) {
                        int j = wj[q];
                        j = j >= 0 && j < UHC_SM_NJ ? j : 0;
                        const double w = ww[q];
#pragma unroll
                        for (int c = 0; c < UHC_SM_XF; c++) Tm[c] += w * G[sm_g_index(j, c, lr)];
                    }
                    double o[3];
                    sm_skin_point(Tm, vp, trans[i], o);
                    wx[i] = o[0], wy[i] = o[1];
                    const double h = uhc_sf_height({o[0], o[1], o[2]}, 0.0, A.floor_z);
                    touch[i] = v_real && uhc_sf_touches(h);
                    if (owned[i] && v_real) {
                        if (A.vert) {
                            double* dst = A.vert + ((size_t)(g0 + r0 + lr) * A.n_vert + v) * 3;
                            dst[0] = row_ok[i] ? o[0] : nan, dst[1] = row_ok[i] ? o[1] : nan, dst[2] = row_ok[i] ? o[2] : nan;
                        }
                        if (uhc_sf_below(h)) pen_sum[i] += h, pen_n[i]++;
                        if (uhc_sf_touches(h)) contact_n[i]++;
                        if (uhc_sf_above(h)) above_n[i]++;
                        z_min[i] = o[2] < z_min[i] ? o[2] : z_min[i];
                    }
                }
                if (A.want_metrics) {
#pragma unroll
                    for (int i = 0; i < 4; i++) {  // row r + 1 of (lane, i): lane + 16, the same register -- for the last group lane - 48, the next register
                        const int pi = i < 3 ? i + 1 : 3;
                        const double nx = __shfl(grp == 0 ? wx[pi] : wx[i], sm_next_lane(lane));
                        const double ny = __shfl(grp == 0 ? wy[pi] : wy[i], sm_next_lane(lane));
                        const int nt = __shfl((int)(grp == 0 ? touch[pi] : touch[i]), sm_next_lane(lane));
                        if (has_next[i] && touch[i] && nt != 0) {
                            const UhcSfV3 w0 = {wx[i], wy[i], 0.0}, w1 = {nx, ny, 0.0};
                            skate_sum[i] += uhc_sf_slide(w0, w1), skate_n[i]++;
                        }
                    }
                }
            }
            __syncthreads();  // keeps the four waves on the same vertex tile: what one loads of posedirs, the others find in the cache
        }
    }

    if (!(active && A.want_metrics)) return;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        UhcSfAcc w;
        // (over the 16 lanes of a row group: every lane ends with the same bits)
        w.pen_sum = uhc_xor_sum<8>(pen_sum[i]), w.skate_sum = uhc_xor_sum<8>(skate_sum[i]);
        const double zm = uhc_xor_min<8>(z_min[i]);
        w.h_min = zm - A.floor_z;  // (rounding is monotone: the minimum of the heights is the height of the lowest vertex)
        w.pen_n = uhc_xor_sum<8>(pen_n[i]), w.skate_n = uhc_xor_sum<8>(skate_n[i]), w.contact_n = uhc_xor_sum<8>(contact_n[i]), w.above_n = uhc_xor_sum<8>(above_n[i]);
        if (owned[i] && (lane & 15) == 0) {
            const size_t g = (size_t)(g0 + r0 + sm_cd_row(lane, i));
            if (A.zmin) A.zmin[g] = row_ok[i] ? zm : nan;
            if (A.row_out) uhc_sf_store_row(A.row_out + g * UHC_SF_NMETRIC, w, A.n_vert, has_next[i], row_ok[i], next_ok[i]);
        }
    }
}

__global__ void __launch_bounds__(256) uhc_smpl_means_kernel(const MeshArgs A) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= A.n_seq * UHC_SF_NMETRIC) return;
    const int s = idx / UHC_SF_NMETRIC, k = idx % UHC_SF_NMETRIC;
    const int T = sm_rows_of(A, s);
    const long long g0 = sm_start_of(A, s, T);
    if (g0 < 0) return;  // the sequence is skipped (and counted by uhc_smpl_shape_kernel): nothing of it is read or written
    A.seq_means[idx] = uhc_seq_mean(A.row_out, UHC_SF_NMETRIC, k, g0, T - (k == UHC_SF_SKATE ? 1 : 0));  // (the skate: over the T - 1 pairs of rows)
}

// ------------------------------------------------------------------ C-ABI (include/uhc_amd.h)
extern "C" int32_t uhc_smpl_mesh_create(int32_t n_vert, int32_t n_models, const double* h_v_template, const double* h_shapedirs, const double* h_posedirs,
                                        const double* h_J_regressor, const double* h_weights, const int32_t* h_parents, UhcSmplMesh** out) {
    // every check comes before the first HIP call
    REFUSE("uhc_smpl_mesh_create", !out, "out is NULL");
    *out = nullptr;
    REFUSE("uhc_smpl_mesh_create", n_vert < 1 || n_vert > 65535, "n_vert must be 1 .. 65535");
    REFUSE("uhc_smpl_mesh_create", n_models < 1, "n_models < 1");
    REFUSE("uhc_smpl_mesh_create", (long long)n_models * n_vert > 0x7fffffffLL / (3 * UHC_SM_KPAD), "n_models x n_vert is beyond the tables' index range");
    REFUSE("uhc_smpl_mesh_create", !h_v_template, "h_v_template is NULL");
    REFUSE("uhc_smpl_mesh_create", !h_shapedirs, "h_shapedirs is NULL");
    REFUSE("uhc_smpl_mesh_create", !h_posedirs, "h_posedirs is NULL");
    REFUSE("uhc_smpl_mesh_create", !h_J_regressor, "h_J_regressor is NULL");
    REFUSE("uhc_smpl_mesh_create", !h_weights, "h_weights is NULL");
    REFUSE("uhc_smpl_mesh_create", !h_parents, "h_parents is NULL");
    REFUSE("uhc_smpl_mesh_create", !sm_parents_ok(h_parents), "h_parents is no tree rooted at joint 0 with parent[j] < j (parent[0] = -1)");
    const size_t V = (size_t)n_vert, M = (size_t)n_models;
    REFUSE("uhc_smpl_mesh_create", !uhc_all_finite(h_v_template, M * V * 3), "h_v_template holds a non-finite entry");
    REFUSE("uhc_smpl_mesh_create", !uhc_all_finite(h_shapedirs, M * V * 3 * UHC_SM_NBETA), "h_shapedirs holds a non-finite entry");
    REFUSE("uhc_smpl_mesh_create", !uhc_all_finite(h_posedirs, M * V * 3 * UHC_SM_NFEAT), "h_posedirs holds a non-finite entry");
    REFUSE("uhc_smpl_mesh_create", !uhc_all_finite(h_J_regressor, M * UHC_SM_NJ * V), "h_J_regressor holds a non-finite entry");
    REFUSE("uhc_smpl_mesh_create", !uhc_all_finite(h_weights, M * V * UHC_SM_NJ), "h_weights holds a non-finite entry");

    // the tables as the kernel wants them: posedirs by vertex tile and coordinate, K padded; the skin weights as lists without their zeros (adding 0 x changes no sum)
    const int nt = sm_vert_tiles(n_vert);
    const size_t vpad = (size_t)UHC_SM_TILE * nt, nb = sm_b_doubles(n_vert);
    int nw = 1;
    for (size_t i = 0; i < M * V; i++) {
        int n = 0;
        for (int j = 0; j < UHC_SM_NJ; j++) n += h_weights[i * UHC_SM_NJ + j] != 0.0;
        nw = n > nw ? n : nw;
    }
    std::vector<double> packed(M * nb), ww(M * vpad * nw, 0.0);
    std::vector<int> wj(M * vpad * nw, 0);
    for (size_t m = 0; m < M; m++) {
        sm_pack_posedirs(n_vert, h_posedirs + m * V * 3 * UHC_SM_NFEAT, packed.data() + m * nb);
        for (size_t v = 0; v < V; v++) {
            int n = 0;
            for (int j = 0; j < UHC_SM_NJ; j++) {
                const double w = h_weights[(m * V + v) * UHC_SM_NJ + j];
                if (w != 0.0) wj[(m * vpad + v) * nw + n] = j, ww[(m * vpad + v) * nw + n] = w, n++;
            }
        }
    }
    UhcSmplMesh* S = new UhcSmplMesh();
    *S = UhcSmplMesh{};
    S->n_vert = n_vert, S->n_vtiles = nt, S->n_models = n_models, S->nw = nw;
    for (int j = 0; j < UHC_SM_NJ; j++) S->parents[j] = h_parents[j];
    hipError_t e = uhc_upload(&S->d_v_template, h_v_template, M * V * 3);
    if (e == hipSuccess) e = uhc_upload(&S->d_shapedirs, h_shapedirs, M * V * 3 * UHC_SM_NBETA);
    if (e == hipSuccess) e = uhc_upload(&S->d_jreg, h_J_regressor, M * UHC_SM_NJ * V);
    if (e == hipSuccess) e = uhc_upload(&S->d_posedirs, (const double*)packed.data(), M * nb);
    if (e == hipSuccess) e = uhc_upload(&S->d_wj, (const int*)wj.data(), M * vpad * nw);
    if (e == hipSuccess) e = uhc_upload(&S->d_ww, (const double*)ww.data(), M * vpad * nw);
    if (e != hipSuccess) {
        uhc_smpl_mesh_free(S);
        return uhc_internal_set_error((std::string("uhc_smpl_mesh_create: ") + hipGetErrorString(e)).c_str());
    }
    *out = S;
    return 0;
}

extern "C" void uhc_smpl_mesh_free(UhcSmplMesh* S) {
    if (!S) return;
    void* all[] = {S->d_v_template, S->d_shapedirs, S->d_jreg, S->d_posedirs, S->d_wj, S->d_ww, S->d_v_shaped, S->d_J, S->d_rows};
    for (void* p : all)
        if (p) (void)hipFree(p);
    delete S;
}

extern "C" int32_t uhc_smpl_mesh(void* stream, UhcSmplMesh* mesh, int32_t n_seq, const int64_t* d_seq_start, const int32_t* d_seq_rows, int32_t row_cap,
                                 const int32_t* d_seq_model, const double* d_betas, const double* d_pose_aa, int64_t pose_stride, const double* d_trans,
                                 int64_t trans_stride, int64_t n_rows_total, double floor_z, double* d_vert, double* d_joints, double* d_row_out,
                                 double* d_seq_means, double* d_row_zmin, int32_t* d_bad, int32_t* h_bad) {
    REFUSE("uhc_smpl_mesh", !mesh, "mesh is NULL");
    REFUSE("uhc_smpl_mesh", n_seq < 0, "n_seq < 0");
    REFUSE("uhc_smpl_mesh", row_cap <= 0, "row_cap <= 0");
    REFUSE("uhc_smpl_mesh", n_rows_total < 0, "n_rows_total < 0");
    REFUSE("uhc_smpl_mesh", pose_stride < 3 * UHC_SM_NJ, "pose_stride is below 72 (rows would overlap)");
    REFUSE("uhc_smpl_mesh", trans_stride < 3, "trans_stride is below 3 (rows would overlap)");
    REFUSE("uhc_smpl_mesh", pose_stride > (1LL << 31) || trans_stride > (1LL << 31) || n_rows_total > (1LL << 31), "pose_stride, trans_stride or n_rows_total is beyond 2^31");
    REFUSE("uhc_smpl_mesh", !std::isfinite(floor_z), "floor_z is not finite");
    REFUSE("uhc_smpl_mesh", !d_seq_start, "d_seq_start is NULL");
    REFUSE("uhc_smpl_mesh", !d_seq_rows, "d_seq_rows is NULL");
    REFUSE("uhc_smpl_mesh", !d_betas, "d_betas is NULL");
    REFUSE("uhc_smpl_mesh", !d_pose_aa, "d_pose_aa is NULL");
    REFUSE("uhc_smpl_mesh", !d_trans, "d_trans is NULL");
    REFUSE("uhc_smpl_mesh", !d_vert && !d_joints && !d_row_out && !d_seq_means && !d_row_zmin, "every output is NULL (d_vert, d_joints, d_row_out, d_seq_means, d_row_zmin)");
    REFUSE("uhc_smpl_mesh", !d_bad, "d_bad is NULL");
    const int tiles_per_seq = sm_row_tiles(row_cap);
    const long long blocks = ((long long)n_seq * tiles_per_seq + SM_WAVES - 1) / SM_WAVES;
    REFUSE("uhc_smpl_mesh", !uhc_launch_fits(blocks) || !uhc_launch_fits((long long)n_seq * UHC_SM_NJ), "n_seq x row_cap is beyond one launch");
    if (n_seq == 0) {
        if (h_bad) *h_bad = 0;
        return 0;
    }
    // (the check that reads the handle: behind the empty return, still before the first HIP call)
    const long long shape_blocks = (long long)n_seq * (((long long)UHC_SM_TILE * mesh->n_vtiles + 255) / 256);
    REFUSE("uhc_smpl_mesh", !uhc_launch_fits(shape_blocks), "n_seq x n_vert is beyond one launch");
    hipStream_t st = (hipStream_t)stream;
    const size_t vpad = (size_t)UHC_SM_TILE * mesh->n_vtiles;
    if ((size_t)n_seq > mesh->cap_seq) {  // (hipFree waits for the device: no kernel of an earlier call still reads the old buffers)
        if (mesh->d_v_shaped) (void)hipFree(mesh->d_v_shaped);
        if (mesh->d_J) (void)hipFree(mesh->d_J);
        mesh->d_v_shaped = mesh->d_J = nullptr, mesh->cap_seq = 0;
        HIP_OK(hipMalloc((void**)&mesh->d_v_shaped, sizeof(double) * n_seq * vpad * 3));
        HIP_OK(hipMalloc((void**)&mesh->d_J, sizeof(double) * n_seq * UHC_SM_NJ * 3));
        mesh->cap_seq = (size_t)n_seq;
    }
    double* row_out = d_row_out;
    if (d_seq_means && !row_out) {  // the means are taken over the rows' values: they need a place
        if (!mesh->d_rows || (size_t)n_rows_total > mesh->cap_rows) {  // (at least one row: the means kernel never gets a NULL)
            if (mesh->d_rows) (void)hipFree(mesh->d_rows);
            mesh->d_rows = nullptr, mesh->cap_rows = 0;
            HIP_OK(hipMalloc((void**)&mesh->d_rows, sizeof(double) * (size_t)(n_rows_total > 0 ? n_rows_total : 1) * UHC_SF_NMETRIC));
            mesh->cap_rows = (size_t)n_rows_total;
        }
        row_out = mesh->d_rows;
    }
    if (!mesh->lds_set) {
        HIP_OK(hipFuncSetAttribute((const void*)uhc_smpl_mesh_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SM_LDS_BYTES));
        mesh->lds_set = true;
    }
    MeshArgs A = {};
    A.n_vert = mesh->n_vert, A.n_vtiles = mesh->n_vtiles, A.n_models = mesh->n_models, A.nw = mesh->nw, A.n_seq = n_seq, A.row_cap = row_cap;
    A.tiles_per_seq = tiles_per_seq;
    A.want_metrics = row_out || d_row_zmin ? 1 : 0;
    A.want_vert_loop = A.want_metrics || d_vert ? 1 : 0;
    for (int j = 0; j < UHC_SM_NJ; j++) A.parents[j] = mesh->parents[j];
    A.n_rows_total = n_rows_total, A.pose_stride = pose_stride, A.trans_stride = trans_stride, A.floor_z = floor_z;
    A.v_template = mesh->d_v_template, A.shapedirs = mesh->d_shapedirs, A.jreg = mesh->d_jreg, A.posedirs = mesh->d_posedirs, A.ww = mesh->d_ww, A.wj = mesh->d_wj;
    A.seq_start = (const long long*)d_seq_start, A.seq_rows = d_seq_rows, A.seq_model = d_seq_model, A.betas = d_betas, A.pose = d_pose_aa, A.trans = d_trans;
    A.v_shaped = mesh->d_v_shaped, A.J = mesh->d_J;
    A.vert = d_vert, A.joints = d_joints, A.row_out = row_out, A.seq_means = d_seq_means, A.zmin = d_row_zmin, A.bad = d_bad;
    HIP_OK(hipMemsetAsync(d_bad, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(uhc_smpl_shape_kernel, dim3((unsigned)shape_blocks), dim3(256), 0, st, A);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(uhc_smpl_joints_kernel, dim3((unsigned)(UHC_SM_NJ * n_seq)), dim3(256), 0, st, A);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(uhc_smpl_mesh_kernel, dim3((unsigned)blocks), dim3(64 * SM_WAVES), SM_LDS_BYTES, st, A);
    HIP_OK(hipGetLastError());
    if (d_seq_means) {
        hipLaunchKernelGGL(uhc_smpl_means_kernel, dim3((unsigned)((n_seq * UHC_SF_NMETRIC + 255) / 256)), dim3(256), 0, st, A);
        HIP_OK(hipGetLastError());
    }
    return uhc_return_bad(h_bad, d_bad, st);
}
