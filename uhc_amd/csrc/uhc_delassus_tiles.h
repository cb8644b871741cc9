// uhc_delassus_tiles.h -- index maps of the Delassus build on the matrix unit (k_pgs_fast: A = Yhat Yhat^T in 16 x 16 tiles of v_mfma_f64_16x16x4_f64).
// Plain functions of lane, register and block numbers; no device code.  The kernels and tests/delassus_tiles_probe.cpp (host compiler only) read the same maps.
//
//   rows      r = 16 J + g   (row block J < 4, g < 16)
//   dofs      d = 4 p + k    (panel p, k < 4)
//   operands  lane l supplies Yhat[16 J + (l & 15)][4 p + (l >> 4)]: as the A operand that is A[l & 15][k = l >> 4], as the B operand B[k = l >> 4][l & 15] of
//             the transposed block -- ONE gathered value per (row block, panel) serves both sides of a tile of Yhat Yhat^T
//   results   tile (I, J), lane l, register i < 4:  A[16 I + (l >> 4) + 4 i][16 J + (l & 15)]
//   back to lane = row: for a fixed column block I and register i, lane l holds in its four tiles (I, 0 .. 3) the entries A[16 J + (l & 15)][16 I + 4 i + (l >> 4)]
//             (A is symmetric) -- rows of the four lanes {g, g + 16, g + 32, g + 48}, lane l's own row being the one of J = l >> 4.  Transposing the 4 x 4 array
//             (register J) x (16-lane group l >> 4) with two rounds of half / quarter swaps leaves lane l with A[l][16 I + 4 i + k2] in register k2.
#pragma once
#if defined(__HIP__)  // (the HIP language mode of the compiler; a host-only translation unit sees plain inline functions)
#define UHC_DT_FN __host__ __device__ inline
#else
#define UHC_DT_FN inline
#endif

#define UHC_DT_TILE 16   // rows and columns of a tile
#define UHC_DT_PANEL 4   // dofs per matrix instruction
#define UHC_DT_BLOCKS 4  // row blocks of a 64-row solve

UHC_DT_FN int dt_row_blocks(int nefc) { return (nefc + UHC_DT_TILE - 1) / UHC_DT_TILE; }
UHC_DT_FN int dt_panels(int nv) { return (nv + UHC_DT_PANEL - 1) / UHC_DT_PANEL; }
// A / B operand: the row (A) or column (B) inside the tile and the k index a lane supplies
UHC_DT_FN int dt_ab_index(int lane) { return lane & 15; }
UHC_DT_FN int dt_ab_k(int lane) { return lane >> 4; }
// C / D: row and column inside the tile of register i of a lane
UHC_DT_FN int dt_cd_row(int lane, int i) { return (lane >> 4) + 4 * i; }
UHC_DT_FN int dt_cd_col(int lane) { return lane & 15; }
// the gather: row of Yhat and dof a lane supplies for row block J and panel p
UHC_DT_FN int dt_gather_row(int J, int lane) { return UHC_DT_TILE * J + dt_ab_index(lane); }
UHC_DT_FN int dt_gather_dof(int p, int lane) { return UHC_DT_PANEL * p + dt_ab_k(lane); }

// A packed row lies along the dof chain of its last dof, ordered from the root; dofs are numbered depth-first, so the chain's dofs ascend and the
// position of dof d on it is the number of chain dofs below d.  mask: bit d of (lo, hi) = dof d is on the chain (nv <= 128).  -> position, or -1: not on it.
// (A dense row is the chain of all nv dofs: dt_all_dofs.)
UHC_DT_FN int dt_popcount64(unsigned long long x) { return __builtin_popcountll(x); }
UHC_DT_FN int dt_chain_pos(unsigned long long lo, unsigned long long hi, int d) {
    if (d < 0 || d >= 128) return -1;
    const unsigned long long w = d < 64 ? lo : hi;
    const int sh = d & 63;
    if (!((w >> sh) & 1ull)) return -1;
    return dt_popcount64(w & ((1ull << sh) - 1ull)) + (d < 64 ? 0 : dt_popcount64(lo));
}
// the mask of dof i's chain from the parent table (the planner fills DevTopo::dof_chainmask with it)
template <class Int>
UHC_DT_FN void dt_chain_mask(const Int* dof_parentid, int i, unsigned long long* lo, unsigned long long* hi) {
    *lo = *hi = 0ull;
    for (int k = i; k >= 0 && k < 128; k = (int)dof_parentid[k]) *(k < 64 ? lo : hi) |= 1ull << (k & 63);
}
UHC_DT_FN unsigned long long dt_all_dofs(int nv, int word) {  // word 0: dofs 0 .. 63, word 1: dofs 64 .. 127
    const int n = nv - 64 * word;
    return n <= 0 ? 0ull : n >= 64 ? ~0ull : (1ull << n) - 1ull;
}

// the two exchanges of gfx950 the transposition is made of, as maps: after swap(x, y) lane l of x / of y holds what lane dt_swap*_lane(l) of register
// dt_swap*_reg(l, 0 / 1) (0 = x, 1 = y) held before.
//   32: lanes 32 .. 63 of x <-> lanes 0 .. 31 of y           16: the odd 16-lane groups of x <-> the even ones of y
UHC_DT_FN int dt_swap32_reg(int lane, int which) { return which == 0 ? (lane >= 32 ? 1 : 0) : (lane < 32 ? 0 : 1); }
UHC_DT_FN int dt_swap32_lane(int lane, int which) { return which == 0 ? (lane >= 32 ? lane - 32 : lane) : (lane < 32 ? lane + 32 : lane); }
UHC_DT_FN int dt_swap16_reg(int lane, int /*which*/) { return (lane >> 4) & 1; }  // (both end with x's words in their even groups and y's in their odd ones)
UHC_DT_FN int dt_swap16_lane(int lane, int which) { return which == 0 ? (((lane >> 4) & 1) ? lane - 16 : lane) : (((lane >> 4) & 1) ? lane : lane + 16); }
// the transposition is swap32(v0, v2), swap32(v1, v3), swap16(v0, v1), swap16(v2, v3); afterwards register k2 of lane l holds what register
// l >> 4 of lane 16 k2 + (l & 15) held, which for the tiles (I, 0 .. 3) at register i is column dt_out_col(I, i, k2) of row l
UHC_DT_FN int dt_tr_src_lane(int lane, int k2) { return 16 * k2 + (lane & 15); }
UHC_DT_FN int dt_tr_src_reg(int lane) { return lane >> 4; }
UHC_DT_FN int dt_out_col(int I, int i, int k2) { return UHC_DT_TILE * I + 4 * i + k2; }
