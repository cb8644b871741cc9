// delassus_tiles_probe.cpp -- the Delassus build's index maps (uhc_amd/csrc/uhc_delassus_tiles.h) on the CPU, for tests/test_delassus_tiles_cpu.py.
// A stand-alone program, host compiler only: it emulates the 16 x 16 x 4 matrix instruction from the operand / result lane maps, runs
// gather -> tiles -> transposition the way k_pgs_fast does on random trees, rows and dense rows, and compares with the naive double loop.
//   delassus_tiles_probe [topology file ...]      file: "<name> <nv>" and nv parent dofs (-1: a root); the built-in trees are always run
// Prints one line per topology and "OK <cases>"; exit status 1 and the first difference otherwise.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "uhc_delassus_tiles.h"

typedef unsigned long long u64;
static u64 g_rng = 88172645463325252ull;
static u64 rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static int rint_(int n) { return (int)(rnd() % (u64)n); }
static double rval() { return ((double)(rnd() % 2000001ull) - 1000000.0) / 1000000.0; }

struct Tree { std::string name; int nv; std::vector<int> parent; };
// a random forest in depth-first order (a dof's parent is the dof before it or one of that dof's ancestors, or none), chains of at most 32 dofs
static Tree random_tree(const char* name, int nv) {
    Tree t{name, nv, std::vector<int>(nv, -1)};
    std::vector<int> depth(nv, 0);
    for (int i = 1; i < nv; i++) {
        int p = i - 1;
        while (p >= 0 && (rint_(3) == 0 || depth[p] >= 31)) p = t.parent[p];
        t.parent[i] = p;
        depth[i] = p < 0 ? 0 : depth[p] + 1;
    }
    return t;
}
static Tree chain_tree(int nv) {
    Tree t{"chain" + std::to_string(nv), nv, std::vector<int>(nv, -1)};
    for (int i = 1; i < nv; i++) t.parent[i] = i - 1;
    return t;
}
static std::vector<int> chain_of(const Tree& t, int i) {  // from the root (DevTopo::dof_anc)
    std::vector<int> c;
    for (int k = i; k >= 0; k = t.parent[k]) c.push_back(k);
    std::reverse(c.begin(), c.end());
    return c;
}

static int fail(const char* what, const Tree& t, int a, int b, double x, double y) {
    printf("FAIL %s: tree %s (nv %d) at (%d, %d): %.17g vs %.17g\n", what, t.name.c_str(), t.nv, a, b, x, y);
    return 1;
}

// the position table against the chains: every (dof, ancestor) pair, and every dof that is not an ancestor
static int check_masks(const Tree& t) {
    for (int i = 0; i < t.nv; i++) {
        u64 lo, hi;
        dt_chain_mask(t.parent.data(), i, &lo, &hi);
        const std::vector<int> c = chain_of(t, i);
        std::vector<int> want(128, -1);
        for (int q = 0; q < (int)c.size(); q++) want[c[q]] = q;
        for (int d = -1; d <= 128; d++) {
            const int w = (d >= 0 && d < 128) ? want[d] : -1;
            if (dt_chain_pos(lo, hi, d) != w) return fail("chain position", t, i, d, dt_chain_pos(lo, hi, d), w);
        }
    }
    return 0;
}

struct Row { int last, yoff, two; };  // FastRow's fields of the build
static int run_case(const Tree& t, int nefc, int ndense, int* cases) {
    const int nv = t.nv, nvp = (nv + 1) & ~1;
    // ---- rows: random last dof (now and then none), packed entries; dense rows at lane 0, lane nefc - 1 and random lanes
    std::vector<Row> row(64, Row{0, 0, -1});
    std::vector<double> S;  // the LDS image: packed rows, then the dense rows
    std::vector<int> dense_lane;
    if (ndense > 0) dense_lane.push_back(0);
    if (ndense > 1 && nefc > 1) dense_lane.push_back(nefc - 1);
    while ((int)dense_lane.size() < std::min(ndense, nefc)) {
        const int l = rint_(nefc);
        if (std::find(dense_lane.begin(), dense_lane.end(), l) == dense_lane.end()) dense_lane.push_back(l);
    }
    std::vector<std::vector<double>> full(64, std::vector<double>(128, 0.0));  // the naive expansion of every row over the dofs
    for (int r = 0; r < nefc; r++) {
        const auto it = std::find(dense_lane.begin(), dense_lane.end(), r);
        if (it != dense_lane.end()) { row[r] = Row{-1, (int)S.size(), (int)(it - dense_lane.begin())}; continue; }
        const int last = rint_(12) == 0 ? -1 : rint_(nv);
        row[r] = Row{last, (int)S.size(), -1};
        if (last < 0) continue;
        const std::vector<int> c = chain_of(t, last);
        for (int q = 0; q < (int)c.size(); q++) { const double y = rint_(9) == 0 ? 0.0 : rval(); S.push_back(y); full[r][c[q]] = y; }
    }
    for (int r = nefc; r < 64; r++) row[r] = Row{rint_(nv), rint_(std::max(1, (int)S.size())), rint_(2) ? rint_(4) : -1};  // lanes past the rows: anything, never used
    S.push_back(777.0);  // (the slack entry a gather may stand on)
    const int Ybase = 0, Dbase = (int)S.size();
    for (int k = 0; k < (int)dense_lane.size(); k++)
        for (int d = 0; d < nvp; d++) { const double y = (d < nv && rint_(4) != 0) ? rval() : (d < nv ? 0.0 : 555.0); S.push_back(y); if (d < nv) full[dense_lane[k]][d] = y; }
    S.push_back(999.0);
    // ---- the build, as k_pgs_fast walks it
    const int nblk = dt_row_blocks(nefc), npan = dt_panels(nv);
    int gbase[4][64]; u64 gm0[4][64], gm1[4][64];
    for (int J = 0; J < 4; J++)
        for (int l = 0; l < 64; l++) {
            gbase[J][l] = Ybase; gm0[J][l] = gm1[J][l] = 0;
            const int src = dt_gather_row(J, l);
            if (J >= nblk || src >= nefc) continue;
            const Row& s = row[src];
            if (s.two >= 0) { gbase[J][l] = Dbase + s.two * nvp; gm0[J][l] = dt_all_dofs(nv, 0); gm1[J][l] = dt_all_dofs(nv, 1); }
            else if (s.last >= 0) { gbase[J][l] = Ybase + s.yoff; dt_chain_mask(t.parent.data(), s.last, &gm0[J][l], &gm1[J][l]); }
        }
    std::vector<std::vector<double>> got(64, std::vector<double>(64, 0.0));
    std::vector<std::vector<double>> seen(64, std::vector<double>(128, 0.0));  // what the gathers supplied, by (row, dof)
    for (int I = 0; I < 4; I++) {
        double acc[4][64][4] = {};
        if (I < nblk) {
            for (int h = 0; h < 2; h++) {
                const int p0 = 16 * h, p1 = std::min(npan, 16 * h + 16);
                if (p0 >= p1) break;
                u64 rmk[4][64]; int at[4][64];
                for (int J = 0; J < 4; J++)
                    for (int l = 0; l < 64; l++) {
                        const int kq = dt_ab_k(l);
                        const u64 wd = h ? gm1[J][l] : gm0[J][l];
                        at[J][l] = gbase[J][l] + dt_popcount64(wd & ((1ull << kq) - 1ull)) + (h ? dt_popcount64(gm0[J][l]) : 0);
                        rmk[J][l] = wd >> kq;
                    }
                for (int p = p0; p <= p1; p++) {  // (p1: the gather ahead of the last panel, read and not used)
                    double v[4][64] = {};
                    for (int J = 0; J < nblk; J++)
                        for (int l = 0; l < 64; l++) {
                            if (at[J][l] < 0 || at[J][l] >= (int)S.size()) return fail("gather out of bounds", t, J, l, at[J][l], (double)S.size());
                            const double x = S[at[J][l]];
                            v[J][l] = (rmk[J][l] & 1ull) ? x : 0.0;
                            at[J][l] += dt_popcount64(rmk[J][l] & 15ull);
                            rmk[J][l] >>= UHC_DT_PANEL;
                            if (p < p1 && I == 0) seen[dt_gather_row(J, l)][dt_gather_dof(p, l)] = v[J][l];
                        }
                    if (p == p1) break;
                    for (int J = 0; J < nblk; J++)  // D += A B: A[m][k] from the lane with (index m, k), B[k][n] likewise from the other block
                        for (int l = 0; l < 64; l++)
                            for (int i = 0; i < 4; i++) {
                                const int m = dt_cd_row(l, i), n = dt_cd_col(l);
                                double sum = acc[J][l][i];
                                for (int k = 0; k < 4; k++) sum = std::fma(v[I][16 * k + m], v[J][16 * k + n], sum);  // lane 16 k + m: dt_ab_index = m, dt_ab_k = k
                                acc[J][l][i] = sum;
                            }
                }
            }
        }
        for (int i = 0; i < 4; i++) {
            double reg[4][64], tmp[4][64];
            for (int J = 0; J < 4; J++) for (int l = 0; l < 64; l++) reg[J][l] = acc[J][l][i];
            auto swap = [&](int x, int y, bool half) {
                const int xy[2] = {x, y};
                for (int l = 0; l < 64; l++)
                    for (int wch = 0; wch < 2; wch++)
                        tmp[xy[wch]][l] = half ? reg[xy[dt_swap32_reg(l, wch)]][dt_swap32_lane(l, wch)] : reg[xy[dt_swap16_reg(l, wch)]][dt_swap16_lane(l, wch)];
                for (int l = 0; l < 64; l++) { reg[x][l] = tmp[x][l]; reg[y][l] = tmp[y][l]; }
            };
            double before[4][64];
            for (int J = 0; J < 4; J++) for (int l = 0; l < 64; l++) before[J][l] = reg[J][l];
            swap(0, 2, true); swap(1, 3, true); swap(0, 1, false); swap(2, 3, false);
            for (int k2 = 0; k2 < 4; k2++)
                for (int l = 0; l < 64; l++) {
                    if (reg[k2][l] != before[dt_tr_src_reg(l)][dt_tr_src_lane(l, k2)]) return fail("transposition map", t, k2, l, reg[k2][l], before[dt_tr_src_reg(l)][dt_tr_src_lane(l, k2)]);
                    got[l][dt_out_col(I, i, k2)] = reg[k2][l];
                }
        }
    }
    // ---- against the naive forms: the gathered entries exactly (same (row, dof) index set, same values), A to 1e-15 of the sum of the products' magnitudes
    for (int r = 0; r < 16 * nblk; r++)
        for (int d = 0; d < 4 * npan; d++)
            if (seen[r][d] != full[r][d]) return fail("gathered entry", t, r, d, seen[r][d], full[r][d]);
    for (int r = 0; r < 64; r++)
        for (int s = 0; s < 64; s++) {
            double ref = 0.0, mag = 0.0;
            if (r < nefc && s < nefc) {
                const Row &a = row[r], &b = row[s];
                if (a.two < 0 && b.two < 0) {  // the common prefix of the two chains
                    if (a.last >= 0 && b.last >= 0) {
                        const std::vector<int> ca = chain_of(t, a.last), cb = chain_of(t, b.last);
                        for (int q = 0; q < (int)std::min(ca.size(), cb.size()) && ca[q] == cb[q]; q++) { const double x = S[Ybase + a.yoff + q] * S[Ybase + b.yoff + q]; ref += x; mag += std::fabs(x); }
                    }
                } else for (int d = 0; d < nv; d++) { const double x = full[r][d] * full[s][d]; ref += x; mag += std::fabs(x); }
            }
            // (no product at all -- no common dof, a row past nefc -- must come out as exactly 0.0: 1e-15 * 0)
            if (!(std::fabs(got[r][s] - ref) <= 1e-15 * mag)) return fail("A entry", t, r, s, got[r][s], ref);
            if (got[r][s] != got[s][r]) return fail("symmetry", t, r, s, got[r][s], got[s][r]);
        }
    ++*cases;
    return 0;
}

int main(int argc, char** argv) {
    std::vector<Tree> trees = {chain_tree(32), random_tree("rand1", 1), random_tree("rand6", 6), random_tree("rand75", 75), random_tree("rand99", 99), random_tree("rand128", 128)};
    for (int a = 1; a < argc; a++) {
        FILE* f = fopen(argv[a], "r");
        char name[64];
        Tree t;
        if (!f || fscanf(f, "%63s %d", name, &t.nv) != 2 || t.nv < 1 || t.nv > 128) { printf("FAIL: cannot read %s\n", argv[a]); return 1; }
        t.name = name; t.parent.assign(t.nv, -1);
        for (int i = 0; i < t.nv; i++)
            if (fscanf(f, "%d", &t.parent[i]) != 1 || t.parent[i] >= i || t.parent[i] < -1) { printf("FAIL: bad parent table in %s\n", argv[a]); return 1; }
        fclose(f);
        trees.push_back(t);
    }
    const int nefcs[] = {1, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64};
    int cases = 0;
    for (const Tree& t : trees) {
        if (check_masks(t)) return 1;
        for (int nefc : nefcs)
            for (int nd = 0; nd <= 5; nd += (nd == 0 ? 2 : 3))  // 0, 2, 5 dense rows (lane 0 and lane nefc - 1 first)
                for (int rep = 0; rep < 2; rep++)
                    if (run_case(t, nefc, nd, &cases)) return 1;
        printf("tree %-10s nv %3d: chain positions and %d builds so far agree\n", t.name.c_str(), t.nv, cases);
    }
    printf("OK %d\n", cases);
    return 0;
}
