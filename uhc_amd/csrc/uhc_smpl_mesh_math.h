// uhc_smpl_mesh_math.h -- the arithmetic and the index maps of the SMPL body mesh (uhc_smpl_mesh.hip; reference: SMPL_Parser.get_joints_verts,
// uhc/smpllib/smpl_parser.py:335-360, which calls smplx's lbs), shared by the device kernel and a host build (tests/smpl_mesh_probe.cpp: the same pieces,
// the matrix product as plain loops).  Straight-line float64, products and sums rounded separately; nothing of the HIP runtime.
//
//   sm_rodrigues     R = I + sin(a) K + (1 - cos(a)) K K,  a = |r + 1e-8|, K = skew(r / a): no branch, R is exactly I at r = 0 (the direction is 0)
//   sm_compose       G_j = G_parent [R_j | J_j - J_parent]: rotation and translation of the chain, one link
//   sm_rest_shift    A_j.t = G_j.t - G_j.R J_j: the transform of REST-pose points
//   sm_skin_point    vertex = T [v; 1] + trans, T = sum_j w_j A_j as 12 doubles (R row-major, then t)
//   feature          k = 9 (j - 1) + e (joint j = 1 .. 23, e = 3 row + column) holds R_j[e] - I[e]; k = 207 is the padding of the K dimension (0)
//
// The pose blend shapes on v_mfma_f64_16x16x4_f64: M = the 16 rows of a row tile, N = the 16 vertices of a vertex tile, K = 208 in 52 steps, one
// accumulator per coordinate.
//   A operand   step p, lane l supplies feature[row sm_a_row(l)][k sm_a_k(p, l)]
//   B operand   step p, lane l supplies posedirs[coordinate c][k sm_b_k(p, l)][vertex 16 vt + sm_b_vert(l)]: the packed table (sm_b_index) puts the 64
//               values of a step next to each other, in lane order
//   C / D       register i < 4 of lane l holds (row sm_cd_row(l, i), vertex sm_cd_vert(l)): x, y and z of ONE vertex for four rows -- skinned where they lie
//   rows        a row tile starts every UHC_SM_OWNED = 15 rows and holds 16: its last row is the first of the next tile, there only as the `next` row of the
//               skate.  Row r + 1 of (lane l, register i) is held by lane sm_next_lane(l) in register sm_next_reg(l, i).
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIP__)  // (the HIP language mode of the compiler; a host-only translation unit sees plain inline functions)
#define UHC_SM_FN __host__ __device__ inline
#else
#define UHC_SM_FN inline
#endif

#define UHC_SM_NJ 24       // joints
#define UHC_SM_NBETA 10    // shape coefficients
#define UHC_SM_NFEAT 207   // 23 x 9
#define UHC_SM_KPAD 208    // the K dimension, padded to the matrix instruction's 4
#define UHC_SM_KSTEPS 52
#define UHC_SM_TILE 16     // rows of a row tile, vertices of a vertex tile
#define UHC_SM_OWNED 15    // rows of a tile whose outputs the tile writes
#define UHC_SM_XF 12       // a transform as doubles: R[9] row-major, t[3]
#define UHC_SM_G_JOINT 193 // doubles between two joints' transforms in a wave's LDS slice: 12 x 16 + 1 (the + 1 spreads the joints over the banks)
#define UHC_SM_G_WAVE (UHC_SM_NJ * UHC_SM_G_JOINT)

UHC_SM_FN void sm_rodrigues(const double* r, double* R) {
    const double ex = r[0] + 1e-8, ey = r[1] + 1e-8, ez = r[2] + 1e-8;
    const double a = sqrt((ex * ex + ey * ey) + ez * ez);
    const double x = r[0] / a, y = r[1] / a, z = r[2] / a;
    const double s = sin(a), c = 1.0 - cos(a);
    // K = [[0, -z, y], [z, 0, -x], [-y, x, 0]];  K K = [[-(yy + zz), xy, xz], [xy, -(xx + zz), yz], [xz, yz, -(xx + yy)]]
    R[0] = 1.0 + c * -(y * y + z * z), R[1] = s * -z + c * (x * y), R[2] = s * y + c * (x * z);
    R[3] = s * z + c * (x * y), R[4] = 1.0 + c * -(x * x + z * z), R[5] = s * -x + c * (y * z);
    R[6] = s * -y + c * (x * z), R[7] = s * x + c * (y * z), R[8] = 1.0 + c * -(x * x + y * y);
}

// are the three numbers finite?  (x - x is 0 for a finite x and NaN for an infinity or a NaN)
UHC_SM_FN bool sm_finite3(const double* v) { return (v[0] - v[0]) + (v[1] - v[1]) + (v[2] - v[2]) == 0.0; }

// (OR | Ot) = (PR | Pt) (R | d)
UHC_SM_FN void sm_compose(const double* PR, const double* Pt, const double* R, const double* d, double* OR, double* Ot) {
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) OR[3 * a + b] = (PR[3 * a] * R[b] + PR[3 * a + 1] * R[3 + b]) + PR[3 * a + 2] * R[6 + b];
        Ot[a] = ((PR[3 * a] * d[0] + PR[3 * a + 1] * d[1]) + PR[3 * a + 2] * d[2]) + Pt[a];
    }
}

UHC_SM_FN void sm_rest_shift(const double* R, const double* t, const double* J, double* out) {
    for (int a = 0; a < 3; a++) out[a] = t[a] - ((R[3 * a] * J[0] + R[3 * a + 1] * J[1]) + R[3 * a + 2] * J[2]);
}

UHC_SM_FN void sm_skin_point(const double* T, const double* v, const double* trans, double* out) {
    for (int a = 0; a < 3; a++) out[a] = (((T[3 * a] * v[0] + T[3 * a + 1] * v[1]) + T[3 * a + 2] * v[2]) + T[9 + a]) + trans[a];
}

// ---- the feature layout
UHC_SM_FN int sm_feat_k(int j, int e) { return 9 * (j - 1) + e; }  // j = 1 .. 23
UHC_SM_FN int sm_feat_joint(int k) { return 1 + k / 9; }           // k < UHC_SM_NFEAT
UHC_SM_FN int sm_feat_elem(int k) { return k % 9; }
UHC_SM_FN double sm_feat_identity(int e) { return e % 4 == 0 ? 1.0 : 0.0; }

// ---- the tiles
UHC_SM_FN int sm_vert_tiles(int n_vert) { return (n_vert + UHC_SM_TILE - 1) / UHC_SM_TILE; }
UHC_SM_FN int sm_row_tiles(int n_rows) { return n_rows <= 0 ? 0 : (n_rows + UHC_SM_OWNED - 1) / UHC_SM_OWNED; }
UHC_SM_FN int sm_tile_row0(int t) { return UHC_SM_OWNED * t; }
UHC_SM_FN int sm_a_row(int lane) { return lane & 15; }
UHC_SM_FN int sm_a_k(int p, int lane) { return 4 * p + (lane >> 4); }
UHC_SM_FN int sm_b_k(int p, int lane) { return 4 * p + (lane >> 4); }
UHC_SM_FN int sm_b_vert(int lane) { return lane & 15; }
UHC_SM_FN int sm_cd_row(int lane, int i) { return (lane >> 4) + 4 * i; }
UHC_SM_FN int sm_cd_vert(int lane) { return lane & 15; }
UHC_SM_FN int sm_next_lane(int lane) { return (lane + 16) & 63; }
UHC_SM_FN int sm_next_reg(int lane, int i) { return i + ((lane >> 4) == 3 ? 1 : 0); }  // (4: beyond the tile -- row 15 has no next row here)
// the packed pose blend shapes of one model: [vertex tile][coordinate][k][vertex in the tile]
UHC_SM_FN size_t sm_b_index(int vt, int c, int k, int vl) { return (((size_t)vt * 3 + c) * UHC_SM_KPAD + k) * UHC_SM_TILE + vl; }
UHC_SM_FN size_t sm_b_doubles(int n_vert) { return (size_t)sm_vert_tiles(n_vert) * 3 * UHC_SM_KPAD * UHC_SM_TILE; }
// a wave's transforms in LDS: (joint, component c < 12, row of the tile)
UHC_SM_FN int sm_g_index(int j, int c, int row) { return j * UHC_SM_G_JOINT + c * UHC_SM_TILE + row; }

// posedirs [n_vert][3][207] (the model file's layout) -> the packed table; padding (k = 207, vertices beyond n_vert) is 0
inline void sm_pack_posedirs(int n_vert, const double* posedirs, double* out) {
    const int nt = sm_vert_tiles(n_vert);
    for (int vt = 0; vt < nt; vt++)
        for (int c = 0; c < 3; c++)
            for (int k = 0; k < UHC_SM_KPAD; k++)
                for (int vl = 0; vl < UHC_SM_TILE; vl++) {
                    const int v = UHC_SM_TILE * vt + vl;
                    out[sm_b_index(vt, c, k, vl)] = v < n_vert && k < UHC_SM_NFEAT ? posedirs[((size_t)v * 3 + c) * UHC_SM_NFEAT + k] : 0.0;
                }
}

// is the parent table a tree rooted at joint 0 with parent[j] < j?
template <class Int>
inline bool sm_parents_ok(const Int* parents) {
    if (parents[0] != -1) return false;
    for (int j = 1; j < UHC_SM_NJ; j++)
        if (parents[j] < 0 || parents[j] >= j) return false;
    return true;
}
