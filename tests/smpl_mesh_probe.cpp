// Host build of uhc_amd/csrc/uhc_smpl_mesh_math.h for tests/test_smpl_mesh_cpu.py: the header's rotation formula, chain, feature layout and tile index maps, with
// the matrix product as plain loops over the operands the maps hand out -- what uhc_smpl_mesh.hip computes with v_mfma_f64_16x16x4_f64.  No HIP header, no hipcc.
#include <vector>

#include "uhc_smpl_mesh_math.h"
#include "uhc_surface_math.h"

#define PROBE_API extern "C" __attribute__((visibility("default")))

// One sequence of T rows of ONE model.  v_template [V][3], shapedirs [V][3][10], posedirs [V][3][207], jreg [24][V], weights [V][24], parents [24], beta [10],
// pose [T][72], trans [T][3].  vert [T][V][3], joints [T][24][3], row_out [T][4] (the skate of the last row is left alone), zmin [T], means [4] (over T, T - 1,
// T, T rows; NaN over none).  Returns the number of rows with a non-finite pose or translation (their outputs are NaN), or -1 for a bad parent table.
PROBE_API int uhc_smpl_mesh_probe_seq(int V, const double* v_template, const double* shapedirs, const double* posedirs, const double* jreg, const double* weights,
                                      const int* parents, const double* beta, const double* pose, const double* trans, int T, double floor_z, double* vert,
                                      double* joints, double* row_out, double* zmin, double* means) {
    if (!sm_parents_ok(parents)) return -1;
    const int nt = sm_vert_tiles(V), vpad = UHC_SM_TILE * nt;
    std::vector<double> packed(sm_b_doubles(V)), vs((size_t)vpad * 3, 0.0), J(UHC_SM_NJ * 3, 0.0);
    sm_pack_posedirs(V, posedirs, packed.data());
    for (int v = 0; v < V; v++)
        for (int c = 0; c < 3; c++) {
            double d = 0.0;
            for (int b = 0; b < UHC_SM_NBETA; b++) d += shapedirs[((size_t)v * 3 + c) * UHC_SM_NBETA + b] * beta[b];
            vs[3 * v + c] = v_template[3 * v + c] + d;
        }
    for (int j = 0; j < UHC_SM_NJ; j++)
        for (int v = 0; v < V; v++)
            for (int c = 0; c < 3; c++) J[3 * j + c] += jreg[(size_t)j * V + v] * vs[3 * v + c];

    std::vector<char> ok(T > 0 ? T : 1, 1);
    int bad = 0;
    for (int t = 0; t < sm_row_tiles(T); t++) {
        const int r0 = sm_tile_row0(t);
        // the tile's 16 rows: local rotations, the feature, the chain (rows beyond the sequence's end: the zero pose)
        std::vector<double> G((size_t)UHC_SM_G_WAVE, 0.0), feat((size_t)UHC_SM_TILE * UHC_SM_KPAD, 0.0), tr(UHC_SM_TILE * 3, 0.0);
        for (int lr = 0; lr < UHC_SM_TILE; lr++) {
            const int r = r0 + lr;
            const bool exists = r < T;
            bool fin = true;
            for (int j = 0; j < UHC_SM_NJ; j++) {
                double r3[3] = {0.0, 0.0, 0.0}, Rl[9];
                if (exists)
                    for (int e = 0; e < 3; e++) r3[e] = pose[(size_t)r * 72 + 3 * j + e];
                fin = fin && sm_finite3(r3);
                sm_rodrigues(r3, Rl);
                for (int e = 0; e < 9; e++) {
                    G[sm_g_index(j, e, lr)] = Rl[e];
                    if (j > 0) feat[(size_t)lr * UHC_SM_KPAD + sm_feat_k(j, e)] = Rl[e] - sm_feat_identity(e);
                }
            }
            if (exists)
                for (int e = 0; e < 3; e++) tr[3 * lr + e] = trans[(size_t)r * 3 + e];
            fin = fin && sm_finite3(&tr[3 * lr]);
            if (exists) ok[r] = fin;
            for (int j = 0; j < UHC_SM_NJ; j++) {
                const int p = parents[j];
                double Rl[9], OR[9], Ot[3];
                for (int e = 0; e < 9; e++) Rl[e] = G[sm_g_index(j, e, lr)];
                if (p < 0) {
                    for (int e = 0; e < 9; e++) OR[e] = Rl[e];
                    for (int e = 0; e < 3; e++) Ot[e] = J[3 * j + e];
                } else {
                    double PR[9], Pt[3], d[3];
                    for (int e = 0; e < 9; e++) PR[e] = G[sm_g_index(p, e, lr)];
                    for (int e = 0; e < 3; e++) Pt[e] = G[sm_g_index(p, 9 + e, lr)], d[e] = J[3 * j + e] - J[3 * p + e];
                    sm_compose(PR, Pt, Rl, d, OR, Ot);
                }
                for (int e = 0; e < 9; e++) G[sm_g_index(j, e, lr)] = OR[e];
                for (int e = 0; e < 3; e++) G[sm_g_index(j, 9 + e, lr)] = Ot[e];
                if (exists && lr < UHC_SM_OWNED)
                    for (int e = 0; e < 3; e++) joints[((size_t)r * UHC_SM_NJ + j) * 3 + e] = fin ? Ot[e] + tr[3 * lr + e] : NAN;
            }
            for (int j = 0; j < UHC_SM_NJ; j++) {
                double Rg[9], tt[3], ts[3];
                for (int e = 0; e < 9; e++) Rg[e] = G[sm_g_index(j, e, lr)];
                for (int e = 0; e < 3; e++) tt[e] = G[sm_g_index(j, 9 + e, lr)];
                sm_rest_shift(Rg, tt, &J[3 * j], ts);
                for (int e = 0; e < 3; e++) G[sm_g_index(j, 9 + e, lr)] = ts[e];
            }
        }
        for (int vt = 0; vt < nt; vt++) {
            double D[3][UHC_SM_TILE][UHC_SM_TILE] = {};  // [coordinate][row][vertex]
            for (int c = 0; c < 3; c++)
                for (int p = 0; p < UHC_SM_KSTEPS; p++) {
                    double Aop[UHC_SM_TILE][4], Bop[4][UHC_SM_TILE];  // what the 64 lanes supply for this step
                    for (int l = 0; l < 64; l++) {
                        Aop[sm_a_row(l)][sm_a_k(p, l) - 4 * p] = feat[(size_t)sm_a_row(l) * UHC_SM_KPAD + sm_a_k(p, l)];
                        Bop[sm_b_k(p, l) - 4 * p][sm_b_vert(l)] = packed[sm_b_index(vt, c, sm_b_k(p, l), sm_b_vert(l))];
                    }
                    for (int m = 0; m < UHC_SM_TILE; m++)
                        for (int n = 0; n < UHC_SM_TILE; n++)
                            for (int k = 0; k < 4; k++) D[c][m][n] += Aop[m][k] * Bop[k][n];
                }
            for (int l = 0; l < 64; l++)
                for (int i = 0; i < 4; i++) {  // lane l, register i: one (row, vertex)
                    const int lr = sm_cd_row(l, i), v = UHC_SM_TILE * vt + sm_cd_vert(l), r = r0 + lr;
                    if (!(lr < UHC_SM_OWNED && r < T && v < V)) continue;
                    const double vp[3] = {vs[3 * v] + D[0][lr][sm_cd_vert(l)], vs[3 * v + 1] + D[1][lr][sm_cd_vert(l)], vs[3 * v + 2] + D[2][lr][sm_cd_vert(l)]};
                    double Tm[UHC_SM_XF] = {}, o[3];
                    for (int j = 0; j < UHC_SM_NJ; j++) {
                        const double w = weights[(size_t)v * UHC_SM_NJ + j];
                        if (w == 0.0) continue;
                        for (int c = 0; c < UHC_SM_XF; c++) Tm[c] += w * G[sm_g_index(j, c, lr)];
                    }
                    sm_skin_point(Tm, vp, &tr[3 * lr], o);
                    for (int e = 0; e < 3; e++) vert[((size_t)r * V + v) * 3 + e] = ok[r] ? o[e] : NAN;
                }
        }
    }
    // the metrics: plain loops in vertex order over the vertices just made
    for (int r = 0; r < T; r++) {
        const bool has_next = r + 1 < T;
        UhcSfAcc a = uhc_sf_acc_zero();
        double zm = HUGE_VAL;
        for (int v = 0; v < V; v++) {
            const double* w0 = vert + ((size_t)r * V + v) * 3;
            const double h0 = uhc_sf_height({w0[0], w0[1], w0[2]}, 0.0, floor_z);
            if (uhc_sf_below(h0)) a.pen_sum += h0, a.pen_n++;
            if (uhc_sf_touches(h0)) a.contact_n++;
            if (uhc_sf_above(h0)) a.above_n++;
            zm = w0[2] < zm ? w0[2] : zm;
            if (has_next) {
                const double* w1 = w0 + (size_t)V * 3;
                if (uhc_sf_touches(h0) && uhc_sf_touches(uhc_sf_height({w1[0], w1[1], w1[2]}, 0.0, floor_z)))
                    a.skate_sum += uhc_sf_slide({w0[0], w0[1], 0.0}, {w1[0], w1[1], 0.0}), a.skate_n++;
            }
        }
        a.h_min = zm - floor_z;
        double* out = row_out + (size_t)r * UHC_SF_NMETRIC;
        zmin[r] = ok[r] ? zm : NAN;
        if (ok[r]) {
            uhc_sf_finish(a, V, has_next, out);
            if (has_next && !ok[r + 1]) out[UHC_SF_SKATE] = NAN;
        } else {
            out[UHC_SF_PEN] = out[UHC_SF_FLOAT] = out[UHC_SF_CONTACT] = NAN;
            if (has_next) out[UHC_SF_SKATE] = NAN;
            bad++;
        }
    }
    for (int k = 0; k < UHC_SF_NMETRIC; k++) {
        const int n = T - (k == UHC_SF_SKATE ? 1 : 0);
        double s = 0.0;
        for (int r = 0; r < n; r++) s += row_out[(size_t)r * UHC_SF_NMETRIC + k];
        means[k] = n > 0 ? s / n : NAN;
    }
    return bad;
}

// the index maps by name: 0 a_row(lane) 1 a_k(p, lane) 2 b_k(p, lane) 3 b_vert(lane) 4 cd_row(lane, i) 5 cd_vert(lane) 6 next_lane(lane) 7 next_reg(lane, i)
// 8 feat_k(j, e) 9 feat_joint(k) 10 feat_elem(k) 11 row_tiles(T) 12 tile_row0(t) 13 vert_tiles(V) 14 g_index(j, c) + row 0
PROBE_API long uhc_smpl_mesh_probe_map(int which, int x, int y) {
    switch (which) {
        case 0: return sm_a_row(y);
        case 1: return sm_a_k(x, y);
        case 2: return sm_b_k(x, y);
        case 3: return sm_b_vert(y);
        case 4: return sm_cd_row(x, y);
        case 5: return sm_cd_vert(x);
        case 6: return sm_next_lane(x);
        case 7: return sm_next_reg(x, y);
        case 8: return sm_feat_k(x, y);
        case 9: return sm_feat_joint(x);
        case 10: return sm_feat_elem(x);
        case 11: return sm_row_tiles(x);
        case 12: return sm_tile_row0(x);
        case 13: return sm_vert_tiles(x);
        case 14: return sm_g_index(x, y, 0);
    }
    return -1;
}

// sm_b_index(vt, c, k, vl), and the packed table of a posedirs [V][3][207] (out: sm_b_doubles(V) doubles; returns that count)
PROBE_API long uhc_smpl_mesh_probe_b_index(int vt, int c, int k, int vl) { return (long)sm_b_index(vt, c, k, vl); }
PROBE_API long uhc_smpl_mesh_probe_pack(int V, const double* posedirs, double* out) {
    if (out) sm_pack_posedirs(V, posedirs, out);
    return (long)sm_b_doubles(V);
}

PROBE_API void uhc_smpl_mesh_probe_rodrigues(const double* r3, double* R9) { sm_rodrigues(r3, R9); }
