// Micro-benchmark of v_mfma_f64_16x16x4_f64 with ONE wave on its SIMD, as the Delassus build of k_pgs_fast runs it:
//   - dependent-accumulate latency (one accumulator, every instruction waits for the one before),
//   - issue rate (four independent accumulators, the tiles (I, 0 .. 3) of one panel),
//   - the same with the build's LDS gathers between the instructions,
//   - the 4 x 4 lane transposition (v_permlane32_swap / v_permlane16_swap) per group of four doubles,
//   - one whole build replayed with stamps of its own: the nest with the column blocks outside (build_like), the nest with the panels outside and all tiles
//     live (build_once, 1 .. 4 row blocks, with and without the tiles pinned to accumulation registers),
//   - gathers with their mask walk behind independent matrix instructions against each alone (overlap),
// and a check of the operand / result lane maps and of the transposition (uhc_amd/csrc/uhc_delassus_tiles.h) on the device: a 64 x 64 product
// Y Y^T built the way the kernel builds it, compared with the host's double loop.
// hipcc --offload-arch=gfx950 -O3 -I../../uhc_amd/csrc mfma_f64.hip -o mfma_f64        cycles = s_memtime ticks (shader clock)
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "uhc_delassus_tiles.h"
#define N 2048
#define NV 76  // 19 panels
typedef double acc4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void swap32(double& x, double& y) {
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
    x = __hiloint2double((int)hi[0], (int)lo[0]); y = __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ void swap16(double& x, double& y) {
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
    x = __hiloint2double((int)hi[0], (int)lo[0]); y = __hiloint2double((int)hi[1], (int)lo[1]);
}
__global__ void k(const double* Yin, double* Aout, double* sink, long long* cyc) {
    __shared__ double Y[64 * NV];
    const int lane = threadIdx.x;
    for (int i = lane; i < 64 * NV; i += 64) Y[i] = Yin[i];
    __syncthreads();
    long long t0, t1;
    double a = Y[lane], b = Y[lane + 64];
    acc4 c0 = {0, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0;
    // 0: dependent accumulate
    t0 = __builtin_readcyclecounter();
#pragma unroll 16
    for (int i = 0; i < N; i++) c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c0, 0, 0, 0);
    t1 = __builtin_readcyclecounter(); if (lane == 0) cyc[0] = t1 - t0;
    // 1: four independent accumulators
    t0 = __builtin_readcyclecounter();
#pragma unroll 4
    for (int i = 0; i < N; i++) {
        c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c0, 0, 0, 0); c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c1, 0, 0, 0);
        c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c2, 0, 0, 0); c3 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c3, 0, 0, 0);
    }
    t1 = __builtin_readcyclecounter(); if (lane == 0) cyc[1] = t1 - t0;
    // 2: four accumulators, four LDS gathers per panel one panel ahead (lane-dependent addresses as in the build)
    {
        int at = (dt_ab_index(lane) * NV + dt_ab_k(lane)) % (64 * NV - 4 * NV);
        double v0 = Y[at], v1 = Y[at + NV], v2 = Y[at + 2 * NV], v3 = Y[at + 3 * NV];
        t0 = __builtin_readcyclecounter();
#pragma unroll 4
        for (int i = 0; i < N; i++) {
            at = (at + 4) & 1023;
            const double n0 = Y[at], n1 = Y[at + NV], n2 = Y[at + 2 * NV], n3 = Y[at + 3 * NV];
            c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(v0, v0, c0, 0, 0, 0); c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(v0, v1, c1, 0, 0, 0);
            c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(v0, v2, c2, 0, 0, 0); c3 = __builtin_amdgcn_mfma_f64_16x16x4f64(v0, v3, c3, 0, 0, 0);
            v0 = n0; v1 = n1; v2 = n2; v3 = n3;
        }
        t1 = __builtin_readcyclecounter(); if (lane == 0) cyc[2] = t1 - t0;
    }
    // 3: the transposition of four doubles (8 swaps of 32 bits)
    double x0 = c0[0], x1 = c1[0], x2 = c2[0], x3 = c3[0];
    t0 = __builtin_readcyclecounter();
#pragma unroll 16
    for (int i = 0; i < N; i++) { swap32(x0, x2); swap32(x1, x3); swap16(x0, x1); swap16(x2, x3); }
    t1 = __builtin_readcyclecounter(); if (lane == 0) cyc[3] = t1 - t0;
    sink[lane] = x0 + x1 + x2 + x3 + c0[1] + c1[2] + c2[3] + c3[1];
    // ---- the maps: A = Y Y^T, 64 rows, NV dofs, by column blocks as in k_pgs_fast; lane r ends with row r
    for (int I = 0; I < 4; I++) {
        acc4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
        for (int p = 0; p < dt_panels(NV); p++) {
            double v[4];
            for (int J = 0; J < 4; J++) { const int d = dt_gather_dof(p, lane); v[J] = d < NV ? Y[dt_gather_row(J, lane) * NV + d] : 0.0; }
            for (int J = 0; J < 4; J++) acc[J] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[I], v[J], acc[J], 0, 0, 0);
        }
        for (int i = 0; i < 4; i++) {
            double t0 = acc[0][i], t1 = acc[1][i], t2 = acc[2][i], t3 = acc[3][i];
            swap32(t0, t2); swap32(t1, t3); swap16(t0, t1); swap16(t2, t3);
            Aout[lane * 64 + dt_out_col(I, i, 0)] = t0; Aout[lane * 64 + dt_out_col(I, i, 1)] = t1;
            Aout[lane * 64 + dt_out_col(I, i, 2)] = t2; Aout[lane * 64 + dt_out_col(I, i, 3)] = t3;
        }
    }
}
// ---- one Delassus build as k_pgs_fast runs it, in three stamped parts: set-up (row fields through ds_bpermute, chain masks from global memory), the tiles of all
//      column blocks (mask walk, gathers a panel ahead, uniform tests of the row-block count), the way back (transposition + 128 AGPR writes).  41 rows of chains of
//      <= 32 dofs among 75: the headline's mean solve.  NBC > 0: the row-block count as a compile-time constant, i.e. the same loops without the uniform tests.
template <int NBC>
__global__ void build_like(const double* Yin, const unsigned long long* masks, const int* rowinfo, int nefc, int nv, double* sink, long long* cyc) {
    __shared__ double Y[64 * 32 + 8];
    const int lane = threadIdx.x;
    for (int i = lane; i < 64 * 32 + 8; i += 64) Y[i] = Yin[i % (64 * NV)];
    __syncthreads();
    const int my_last = rowinfo[lane], my_yoff = 32 * lane;
    long long t0 = __builtin_readcyclecounter();
    const int nblk = NBC > 0 ? NBC : __builtin_amdgcn_readfirstlane(dt_row_blocks(nefc));
    const int npan = dt_panels(nv), kq = dt_ab_k(lane);
    int gbase[4]; unsigned long long gm0[4], gm1[4];
#pragma unroll
    for (int J = 0; J < 4; J++) {
        gbase[J] = 0; gm0[J] = gm1[J] = 0;
        if (J < nblk) {
            const int src = dt_gather_row(J, lane);
            const int s_last = __builtin_amdgcn_ds_bpermute(src << 2, my_last), s_yoff = __builtin_amdgcn_ds_bpermute(src << 2, my_yoff);
            if (src < nefc && s_last >= 0) { gbase[J] = s_yoff; gm0[J] = masks[2 * s_last]; gm1[J] = masks[2 * s_last + 1]; }
        }
    }
    asm volatile("" : "+v"(gbase[0]), "+v"(gbase[1]), "+v"(gbase[2]), "+v"(gbase[3]));
    long long t1 = __builtin_readcyclecounter();
    long long t_tiles = 0, t_back = 0;
    double total = 0;
#pragma unroll
    for (int I = 0; I < 4; I++) {
        if (I >= nblk) continue;
        long long a0 = __builtin_readcyclecounter();
        acc4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
        for (int h = 0; h < 2; h++) {
            const int p0 = 16 * h, p1 = min(npan, 16 * h + 16);
            if (p0 >= p1) break;
            unsigned long long rmk[4]; int at[4];
#pragma unroll
            for (int J = 0; J < 4; J++) {
                const unsigned long long wd = h ? gm1[J] : gm0[J];
                at[J] = gbase[J] + __popcll(wd & ((1ull << kq) - 1ull)) + (h ? __popcll(gm0[J]) : 0);
                rmk[J] = wd >> kq;
            }
            double v[4], vn[4];
#pragma unroll
            for (int J = 0; J < 4; J++) { v[J] = 0; if (J < nblk) { const double x = Y[at[J]]; v[J] = ((unsigned)rmk[J] & 1u) ? x : 0.0; at[J] += __popc((unsigned)rmk[J] & 15u); rmk[J] >>= 4; } }
            for (int p = p0; p < p1; p++) {
#pragma unroll
                for (int J = 0; J < 4; J++) { vn[J] = 0; if (J < nblk) { const double x = Y[at[J]]; vn[J] = ((unsigned)rmk[J] & 1u) ? x : 0.0; at[J] += __popc((unsigned)rmk[J] & 15u); rmk[J] >>= 4; } }
#pragma unroll
                for (int J = 0; J < 4; J++) if (J < nblk) acc[J] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[I], v[J], acc[J], 0, 0, 0);
#pragma unroll
                for (int J = 0; J < 4; J++) v[J] = vn[J];
            }
        }
        asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));
        long long a1 = __builtin_readcyclecounter();
#pragma unroll
        for (int i = 0; i < 4; i++) {
            double x0 = acc[0][i], x1 = acc[1][i], x2 = acc[2][i], x3 = acc[3][i];
            swap32(x0, x2); swap32(x1, x3); swap16(x0, x1); swap16(x2, x3);
            const double w[4] = {x0, x1, x2, x3};
#pragma unroll
            for (int k2 = 0; k2 < 4; k2++) {
                int lo, hi;
                asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(lo) : "v"(__double2loint(w[k2])));
                asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(hi) : "v"(__double2hiint(w[k2])));
                int rl, rh;
                asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(rl) : "a"(lo));
                asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(rh) : "a"(hi));
                total += __hiloint2double(rh, rl);
            }
        }
        asm volatile("" : "+v"(total));
        long long a2 = __builtin_readcyclecounter();
        t_tiles += a1 - a0; t_back += a2 - a1;
    }
    sink[lane] = total;
    if (lane == 0) { cyc[0] = t1 - t0; cyc[1] = t_tiles; cyc[2] = t_back; }
}
// ---- the same build with the loops interchanged, as delassus_tiles<NB> of uhc_physics_impl.h runs it: the panels outside, every row block gathered ONCE per panel,
//      all NB x NB tiles live, the row-block count a template argument; then the way back per column block.  Same three stamps.
//      This is a hand copy of the kernel's code, not an instantiation of it (the kernel's functions take its KernelArgs, FastRow and LDS layout).  What must stay
//      in step with uhc_physics_impl.h for the figures to speak for the kernel: the set-up (k_pgs_fast: two ds_bpermute per row block, masks from global memory),
//      the walk of a gather (delassus_tiles: LDS read at the lane's own offset, select by the mask's low bit, offset += popcount of four bits, mask >>= 4), the
//      gather one panel ahead of its use, the order of the NB x NB instructions (I outer, J inner), the two loops over the mask words, and the way back
//      (delassus_back: per column block four rounds of two swap32 + two swap16, then four columns to the AGPRs).  build_like is the same kind of copy of the nest
//      the kernel had before.
//      PIN: an empty asm statement asks for every tile in an accumulation register where the panel loop is entered and at the end of each panel.  The kernels of
//      this file that use AGPRs (as the step kernels do) get the instruction's AGPR form; without the pin the compiler carries the tiles round the loop in VGPRs and
//      moves all of them to the AGPRs and back in every panel (v_accvgpr_write / _read, each read waiting for its instruction).
template <int NB, bool PIN>
__global__ void __launch_bounds__(64) build_once(const double* Yin, const unsigned long long* masks, const int* rowinfo, int nefc, int nv, double* sink, long long* cyc) {
    __shared__ double Y[64 * 32 + 8];
    const int lane = threadIdx.x;
    for (int i = lane; i < 64 * 32 + 8; i += 64) Y[i] = Yin[i % (64 * NV)];
    __syncthreads();
    const int my_last = rowinfo[lane], my_yoff = 32 * lane;
    long long t0 = __builtin_readcyclecounter();
    const int npan = dt_panels(nv), kq = dt_ab_k(lane);
    int gbase[NB]; unsigned long long gm0[NB], gm1[NB];
#pragma unroll
    for (int J = 0; J < NB; J++) {
        gbase[J] = 0; gm0[J] = gm1[J] = 0;
        const int src = dt_gather_row(J, lane);
        const int s_last = __builtin_amdgcn_ds_bpermute(src << 2, my_last), s_yoff = __builtin_amdgcn_ds_bpermute(src << 2, my_yoff);
        if (src < nefc && s_last >= 0) { gbase[J] = s_yoff; gm0[J] = masks[2 * s_last]; gm1[J] = masks[2 * s_last + 1]; }
    }
#pragma unroll
    for (int J = 0; J < NB; J++) asm volatile("" : "+v"(gbase[J]));
    long long t1 = __builtin_readcyclecounter();
    acc4 acc[4][4];
#pragma unroll
    for (int t = 0; t < 16; t++) acc[t / 4][t % 4] = acc4{0, 0, 0, 0};
    if (PIN) {
#pragma unroll
        for (int t = 0; t < NB * NB; t++) asm("" : "+a"(acc[t / NB][t % NB]));
    }
    for (int h = 0; h < 2; h++) {
        const int p0 = 16 * h, p1 = min(npan, 16 * h + 16);
        if (p0 >= p1) break;
        unsigned long long rmk[NB]; int at[NB];
#pragma unroll
        for (int J = 0; J < NB; J++) {
            const unsigned long long wd = h ? gm1[J] : gm0[J];
            at[J] = gbase[J] + __popcll(wd & ((1ull << kq) - 1ull)) + (h ? __popcll(gm0[J]) : 0);
            rmk[J] = wd >> kq;
        }
        double v[NB], vn[NB];
#pragma unroll
        for (int J = 0; J < NB; J++) { const double x = Y[at[J]]; v[J] = ((unsigned)rmk[J] & 1u) ? x : 0.0; at[J] += __popc((unsigned)rmk[J] & 15u); rmk[J] >>= 4; }
        for (int p = p0; p < p1; p++) {
#pragma unroll
            for (int J = 0; J < NB; J++) { const double x = Y[at[J]]; vn[J] = ((unsigned)rmk[J] & 1u) ? x : 0.0; at[J] += __popc((unsigned)rmk[J] & 15u); rmk[J] >>= 4; }
#pragma unroll
            for (int t = 0; t < NB * NB; t++) acc[t / NB][t % NB] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[t / NB], v[t % NB], acc[t / NB][t % NB], 0, 0, 0);
            if (PIN) {
#pragma unroll
                for (int t = 0; t < NB * NB; t++) asm("" : "+a"(acc[t / NB][t % NB]));
            }
#pragma unroll
            for (int J = 0; J < NB; J++) v[J] = vn[J];
        }
    }
#pragma unroll
    for (int t = 0; t < NB * NB; t++) asm volatile("" : "+v"(acc[t / NB][t % NB]));
    long long a1 = __builtin_readcyclecounter();
    double total = 0;
#pragma unroll
    for (int I = 0; I < NB; I++) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            double x0 = acc[I][0][i], x1 = acc[I][1][i], x2 = acc[I][2][i], x3 = acc[I][3][i];
            swap32(x0, x2); swap32(x1, x3); swap16(x0, x1); swap16(x2, x3);
            const double w[4] = {x0, x1, x2, x3};
#pragma unroll
            for (int k2 = 0; k2 < 4; k2++) {
                int lo, hi;
                asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(lo) : "v"(__double2loint(w[k2])));
                asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(hi) : "v"(__double2hiint(w[k2])));
                int rl, rh;
                asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(rl) : "a"(lo));
                asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(rh) : "a"(hi));
                total += __hiloint2double(rh, rl);
            }
        }
    }
    asm volatile("" : "+v"(total));
    long long a2 = __builtin_readcyclecounter();
    sink[lane] = total;
    if (lane == 0) { cyc[0] = t1 - t0; cyc[1] = a1 - t1; cyc[2] = a2 - a1; }
}
// ---- do the gathers issue in the shadow of the matrix instructions?  One panel = NG gathers with their mask walk (LDS read, select, popcount, shift) and / or NM
//      independent matrix instructions.  MODE 1: the gathers alone; 2: the instructions alone (fixed operands); 3: both, the instructions on the values gathered a panel
//      ahead, as in the build.  PANELS_OV panels, the masks rewound every 16.
#define PANELS_OV 1024
template <int NG, int NM, int MODE>
__global__ void __launch_bounds__(64) overlap(const double* Yin, const unsigned long long* masks, const int* rowinfo, double* sink, long long* cyc) {
    __shared__ double Y[64 * 32 + 8];
    const int lane = threadIdx.x;
    for (int i = lane; i < 64 * 32 + 8; i += 64) Y[i] = Yin[i % (64 * NV)];
    __syncthreads();
    const int kq = dt_ab_k(lane);
    int gbase[NG]; unsigned long long gm[NG];
#pragma unroll
    for (int J = 0; J < NG; J++) { const int src = dt_gather_row(J, lane); gbase[J] = 32 * src; gm[J] = masks[2 * rowinfo[src]]; }
    acc4 acc[NM];
#pragma unroll
    for (int m = 0; m < NM; m++) acc[m] = acc4{0, 0, 0, 0};
    double v[NG], vn[NG];
#pragma unroll
    for (int J = 0; J < NG; J++) v[J] = vn[J] = Y[lane + 64 * J];
    long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < PANELS_OV / 16; it++) {
        unsigned long long rmk[NG]; int at[NG];
#pragma unroll
        for (int J = 0; J < NG; J++) { at[J] = gbase[J] + __popcll(gm[J] & ((1ull << kq) - 1ull)); rmk[J] = gm[J] >> kq; }
        for (int p = 0; p < 16; p++) {
            if (MODE & 1) {
#pragma unroll
                for (int J = 0; J < NG; J++) { const double x = Y[at[J]]; vn[J] = ((unsigned)rmk[J] & 1u) ? x : 0.0; at[J] += __popc((unsigned)rmk[J] & 15u); rmk[J] >>= 4; }
            }
            if (MODE & 2) {
#pragma unroll
                for (int m = 0; m < NM; m++) acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[m % NG], v[(m / NG) % NG], acc[m], 0, 0, 0);
            }
            if (MODE == 1) {
#pragma unroll
                for (int J = 0; J < NG; J++) asm volatile("" :: "v"(vn[J]));
            }
            if (MODE == 3) {
#pragma unroll
                for (int J = 0; J < NG; J++) v[J] = vn[J];
            }
        }
    }
#pragma unroll
    for (int m = 0; m < NM; m++) asm volatile("" : "+v"(acc[m]));
    long long t1 = __builtin_readcyclecounter();
    double total = 0;
#pragma unroll
    for (int m = 0; m < NM; m++) total += acc[m][0] + acc[m][3];
#pragma unroll
    for (int J = 0; J < NG; J++) total += vn[J];
    sink[lane] = total;
    if (lane == 0) cyc[0] = t1 - t0;
}
template <int NG, int NM>
static void overlap_line(const double* dY, const unsigned long long* dm, const int* drow, double* sink, long long* cyc) {
    long long g[3];
    for (int r = 0; r < 3; r++) hipLaunchKernelGGL((overlap<NG, NM, 1>), dim3(1), dim3(64), 0, 0, dY, dm, drow, sink, cyc);
    hipDeviceSynchronize(); hipMemcpy(&g[0], cyc, 8, hipMemcpyDeviceToHost);
    for (int r = 0; r < 3; r++) hipLaunchKernelGGL((overlap<NG, NM, 2>), dim3(1), dim3(64), 0, 0, dY, dm, drow, sink, cyc);
    hipDeviceSynchronize(); hipMemcpy(&g[1], cyc, 8, hipMemcpyDeviceToHost);
    for (int r = 0; r < 3; r++) hipLaunchKernelGGL((overlap<NG, NM, 3>), dim3(1), dim3(64), 0, 0, dY, dm, drow, sink, cyc);
    hipDeviceSynchronize(); hipMemcpy(&g[2], cyc, 8, hipMemcpyDeviceToHost);
    printf("  %d gathers alone %7.1f | %2d instructions alone %7.1f | both %7.1f   (sum %7.1f: %s)\n", NG, g[0] / (double)PANELS_OV, NM, g[1] / (double)PANELS_OV,
           g[2] / (double)PANELS_OV, (g[0] + g[1]) / (double)PANELS_OV, g[2] < 0.5 * (g[0] + g[1]) + 0.5 * (g[0] > g[1] ? g[0] : g[1]) ? "the gathers issue in the shadow" : "they add up");
}
template <int NB>
static void once_line(const double* dY, const unsigned long long* dm, const int* drow, int nefc, int nv, double* sink, long long* cyc) {
    long long g[3][8];
    for (int r = 0; r < 3; r++) hipLaunchKernelGGL(build_like<0>, dim3(1), dim3(64), 0, 0, dY, dm, drow, nefc, nv, sink, cyc);
    hipDeviceSynchronize(); hipMemcpy(g[0], cyc, 64, hipMemcpyDeviceToHost);
    for (int r = 0; r < 3; r++) hipLaunchKernelGGL((build_once<NB, false>), dim3(1), dim3(64), 0, 0, dY, dm, drow, nefc, nv, sink, cyc);
    hipDeviceSynchronize(); hipMemcpy(g[1], cyc, 64, hipMemcpyDeviceToHost);
    for (int r = 0; r < 3; r++) hipLaunchKernelGGL((build_once<NB, true>), dim3(1), dim3(64), 0, 0, dY, dm, drow, nefc, nv, sink, cyc);
    hipDeviceSynchronize(); hipMemcpy(g[2], cyc, 64, hipMemcpyDeviceToHost);
    const int ninst = NB * NB * dt_panels(nv);
    printf("  %d row blocks (%2d rows, %3d instructions)\n", NB, nefc, ninst);
    const char* what[3] = {"column blocks outside (the old nest)", "panels outside", "panels outside, tiles pinned to AGPRs"};
    for (int k = 0; k < 3; k++) printf("      %-40s %6lld | %7lld | %6lld   = %5.1f per instruction in the tiles\n", what[k], g[k][0], g[k][1], g[k][2], g[k][1] / (double)ninst);
}
int main() {
    static double hY[64 * NV], hA[64 * 64];
    srand(1);
    for (int i = 0; i < 64 * NV; i++) hY[i] = (rand() % 2001 - 1000) / 1000.0;
    double *dY, *dA, *sink; long long* cyc;
    hipMalloc(&dY, sizeof hY); hipMalloc(&dA, sizeof hA); hipMalloc(&sink, 64 * 8); hipMalloc(&cyc, 8 * 8);
    hipMemcpy(dY, hY, sizeof hY, hipMemcpyHostToDevice);
    for (int r = 0; r < 2; r++) hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, dY, dA, sink, cyc);
    if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
    long long h[8]; hipMemcpy(h, cyc, sizeof h, hipMemcpyDeviceToHost);
    hipMemcpy(hA, dA, sizeof hA, hipMemcpyDeviceToHost);
    printf("v_mfma_f64_16x16x4_f64, one wave on its SIMD (s_memtime ticks per instruction)\n");
    printf("%-58s %8.1f\n", "dependent accumulate (latency)", h[0] / (double)N);
    printf("%-58s %8.1f\n", "4 independent accumulators (issue rate)", h[1] / (4.0 * N));
    printf("%-58s %8.1f\n", "4 accumulators + 4 LDS gathers a panel ahead", h[2] / (4.0 * N));
    printf("%-58s %8.1f\n", "4 x 4 lane transposition of 4 doubles (8 swaps), per group", h[3] / (double)N);
    double worst = 0;
    for (int r = 0; r < 64; r++)
        for (int s = 0; s < 64; s++) {
            double ref = 0;
            for (int d = 0; d < NV; d++) ref += hY[r * NV + d] * hY[s * NV + d];
            worst = fmax(worst, fabs(hA[r * 64 + s] - ref));
        }
    printf("lane maps: 64 x 64 product by tiles + transposition vs host, max |diff| = %.3e  %s\n", worst, worst < 1e-12 ? "OK" : "WRONG");
    {   // one build of 41 rows x 75 dofs: every dof's chain = the six root dofs + up to 15 dofs ending at it
        const int nefc = 41, nv = 75;
        static unsigned long long hm[2 * 128];
        static int hrow[64];
        for (int d = 0; d < nv; d++) {
            unsigned long long lo = 0, hi = 0;
            for (int a = 0; a <= d; a++) if (a < 6 || a >= d - 14) *(a < 64 ? &lo : &hi) |= 1ull << (a & 63);
            hm[2 * d] = lo; hm[2 * d + 1] = hi;
        }
        for (int r = 0; r < 64; r++) hrow[r] = (r * 13) % nv;
        unsigned long long* dm; int* drow;
        hipMalloc(&dm, sizeof hm); hipMalloc(&drow, sizeof hrow);
        hipMemcpy(dm, hm, sizeof hm, hipMemcpyHostToDevice); hipMemcpy(drow, hrow, sizeof hrow, hipMemcpyHostToDevice);
        long long g[2][8];
        for (int r = 0; r < 3; r++) hipLaunchKernelGGL(build_like<0>, dim3(1), dim3(64), 0, 0, dY, dm, drow, nefc, nv, sink, cyc);
        hipDeviceSynchronize(); hipMemcpy(g[0], cyc, 64, hipMemcpyDeviceToHost);
        for (int r = 0; r < 3; r++) hipLaunchKernelGGL(build_like<3>, dim3(1), dim3(64), 0, 0, dY, dm, drow, nefc, nv, sink, cyc);
        if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
        hipMemcpy(g[1], cyc, 64, hipMemcpyDeviceToHost);
        printf("one build, 41 rows x 75 dofs (3 row blocks, 19 panels, 171 instructions), s_memtime ticks:  set-up | tiles | back to lane = row (+ AGPR write and read-back)\n");
        printf("  row-block count tested at run time (as the kernel)   %7lld | %7lld | %7lld   = %.1f per instruction in the tiles\n", g[0][0], g[0][1], g[0][2], g[0][1] / 171.0);
        printf("  row-block count a compile-time 3 (no uniform tests)  %7lld | %7lld | %7lld   = %.1f per instruction in the tiles\n", g[1][0], g[1][1], g[1][2], g[1][1] / 171.0);
        printf("one build at nv = 75, every row block gathered once per panel and all tiles live (delassus_tiles<NB>) beside the nest above:  set-up | tiles | back\n");
        once_line<1>(dY, dm, drow, 9, nv, sink, cyc);
        once_line<2>(dY, dm, drow, 25, nv, sink, cyc);
        once_line<3>(dY, dm, drow, 41, nv, sink, cyc);
        once_line<4>(dY, dm, drow, 57, nv, sink, cyc);
        printf("one panel: gathers with their mask walk behind independent matrix instructions, s_memtime ticks per panel\n");
        overlap_line<3, 9>(dY, dm, drow, sink, cyc);
        overlap_line<4, 16>(dY, dm, drow, sink, cyc);
        if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
    }
    return worst < 1e-12 ? 0 : 2;
}
