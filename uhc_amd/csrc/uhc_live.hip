// Live targets: one expert frame record per env and control step, appended to the env's own stream: uhc_env_live_push (include/uhc_amd.h).
//
// The per-env, per-step form of uhc_expert.hip: the same record (uhc_expert_math.h), from the pair (the env's previous row, the pushed row) instead of two
// rows of a bank found by a binary search (the model index is brought into its range by the same rule, uhc_seq.h), written to slot `len` of the env's stream in the live bank [n_env][cap][UHC_FRAME_STRIDE], with the per-env
// bookkeeping the env kernels read (e_len, e_start, clip_id, height_lb).  The entry points and the memory are uhc_env_capi.cpp's.
//
// Mapping: one wave per TWO rows (lanes 0 .. 31 the even one, lanes 32 .. 63 the odd one), four waves per workgroup; within a half, lane = body.  A half
// whose row is ignored (env outside the batch) or dropped (no stream, or a full one) computes the wave's first row along and stores nothing: what the
// halves do differs in data, not in control flow, and every wave reaches the barrier.  After the barrier the half copies its record out of LDS, 16 B per
// lane to consecutive addresses (292 x 16 B), and -- when the row is the stream's frame 1 -- the 75 + 72 velocity slots into frame 0 as well (the
// cat((qvel[0:1], qvel)) rule); its lanes then write the row to prev_qpos, and one lane the counters.
//
// Sliding (uhc_env_live_slide; the rule is uhc_live_window.h's): uhc_live_slide_kernel runs in front of the push kernel, on the same stream, one wave per
// listed row.  Where the env's slice is full and the env has moved on, it discards the S records behind the consumer, moves the others to the front of the
// slice and subtracts S from live_len, e_len and start_ind; the push kernel then finds room and appends as ever.  A kernel of its own, not a phase of the
// push kernel: the move wants a whole wave per env (the push kernel gives a row half a wave, and its halves must not diverge ahead of its barrier), the push
// kernel keeps its registers, and with sliding off nothing at all is launched or read in addition.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uhc_amd.h"
#include "uhc_device_env.h"
#include "uhc_expert_math.h"
#include "uhc_internal.h"
#include "uhc_live_window.h"
#include "uhc_seq.h"

#pragma clang fp contract(off)

#define LV_WAVES 4  // waves per workgroup: eight rows

struct LiveArgs {
    // the call
    const int* env_ids;         // [n]
    const double* qpos;         // [n][76]
    const double* root_record;  // [n][4] or NULL
    const int* restart;         // [n] or NULL
    const int* model;           // [n] or NULL
    int n;
    // the live state (owned by the UhcEnv)
    double* bank;       // [n_env][cap][UHC_FRAME_STRIDE]
    double* prev_qpos;  // [n_env][76]: the stream's newest row, with its OWN root quaternion
    int* live_len;      // [n_env]
    int* dropped;       // [n_env]
    int* live_base;     // [n_env]: frames slid off since the restart (global frame = live_base + local index); 0 while sliding is off
    int* live_moved;    // [n_env]: records copied by slides since the restart
    const double* body_pos;   // [n_models][24][3]
    const double* body_ipos;  // [n_models][24][3]
    int n_env, cap, n_models;
    double dt;
    XfTree tree;
    // what the env kernels read (EnvArgs)
    int *e_len, *e_start, *clip_id, *env_model;  // (env_model: NULL on a batch with one model)
    double* height_lb;
};

__global__ void __launch_bounds__(64 * LV_WAVES) uhc_live_push_kernel(const LiveArgs A) {
    __shared__ __attribute__((aligned(16))) double rec_s[2 * LV_WAVES][UHC_FRAME_STRIDE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, body = lane & 31;
    const int r0 = (blockIdx.x * LV_WAVES + wave) * 2;  // the wave's rows: r0 (lanes 0 .. 31) and r0 + 1 (lanes 32 .. 63)
    const bool wave_valid = r0 < A.n;                   // (wave-uniform; the barrier below is reached by every wave)
    double* rec = rec_s[2 * wave + half];
    // what the half does with its row (half-uniform): 0 nothing, 1 restart, 2 append, 3 drop
    int what = 0, env = 0, L = 0, m = 0;
    const double* row = A.qpos;
    if (wave_valid) {
        const int r = r0 + half < A.n ? r0 + half : r0;  // (the last row may have no partner)
        row = A.qpos + (size_t)r * XF_NQ;
        const int id = A.env_ids[r];
        const bool ok = r0 + half < A.n && id >= 0 && id < A.n_env;  // (no read or write goes through an index outside the batch)
        env = ok ? id : 0;
        if (ok) {
            L = A.live_len[env];
            what = A.restart && A.restart[r] ? 1 : (L >= 1 && L < A.cap ? 2 : 3);
            m = what == 1 && A.model ? A.model[r] : (A.env_model ? A.env_model[env] : 0);
            m = uhc_seq_model(m, A.n_models);
        }
        // the pair: (previous row, row) of an append; a restart is a clip of one frame, and so is what a half computes along
        const bool append = what == 2;
        const double* row_a = append ? A.prev_qpos + (size_t)env * XF_NQ : row;
        const bool store = what == 1 || what == 2;
        xf_half_record(A.tree, A.dt, row_a, row, !append, append, A.root_record && store ? A.root_record + (size_t)r * 4 : nullptr,
                       A.body_pos + (size_t)m * XF_NBODY * 3, A.body_ipos + (size_t)m * XF_NBODY * 3, store, lane, rec);
    }
    __syncthreads();
    if (what == 1 || what == 2) {
        const int slot = what == 1 ? 0 : L;  // 0 <= slot < cap
        double* stream0 = A.bank + (size_t)env * A.cap * UHC_FRAME_STRIDE;
        // the half's record: one run of consecutive 16-byte stores (4 672 B per record: 16-byte aligned)
        const double2* src = reinterpret_cast<const double2*>(rec);
        double2* dst = reinterpret_cast<double2*>(stream0 + (size_t)slot * UHC_FRAME_STRIDE);
        for (int j = body; j < UHC_FRAME_STRIDE / 2; j += 32) dst[j] = src[j];
        // GLOBAL frame 0 takes frame 1's velocities (a dry stream that slid down to one record has L == 1 again: slot 0 is a later frame and keeps its own)
        if (what == 2 && L == 1 && A.live_base[env] == 0) {
            for (int j = body; j < 75; j += 32) stream0[UHC_FR_QVEL + j] = rec[UHC_FR_QVEL + j];
            for (int j = body; j < 72; j += 32) stream0[UHC_FR_BANGVEL + j] = rec[UHC_FR_BANGVEL + j];
        }
        for (int j = body; j < XF_NQ; j += 32) A.prev_qpos[(size_t)env * XF_NQ + j] = row[j];  // (every read of the previous row lies before the barrier)
        if (body == 0) {
            const double h = row[2];
            A.live_len[env] = slot + 1;
            A.e_len[env] = slot + 1;
            if (what == 1) {
                A.e_start[env] = env * A.cap;
                A.clip_id[env] = env;
                A.height_lb[env] = h;
                A.dropped[env] = 0;
                A.live_base[env] = 0;
                A.live_moved[env] = 0;
                if (A.model && A.env_model) A.env_model[env] = m;
            } else {
                A.height_lb[env] = fmin(A.height_lb[env], h);
            }
        }
    } else if (what == 3 && body == 0) {
        A.dropped[env] += 1;
    }
}

// ---------------------------------------------------------------------------------------------------------
// The slide of the listed envs, ahead of the append.  One wave per row, LV_WAVES rows per workgroup; no LDS, no barrier.  A row outside the list's length, a
// foreign id, a restart row (the stream is about to be replaced), a slice that is not full and a consumer that has not moved leave by a wave-uniform early exit
// without a write.  No pointer here is __restrict__: source and destination are the same slice.
#define LV_REC16 (UHC_FRAME_STRIDE / 2)             // a record in 16-byte columns: 292
static_assert(LV_REC16 > 256 && LV_REC16 <= 320, "five columns per lane: four whole ones and a tail on lanes 0 .. LV_REC16 - 257");
__global__ void __launch_bounds__(64 * LV_WAVES) uhc_live_slide_kernel(const int* env_ids, const int* restart, int n, double* bank, int* live_len, int* live_base,
                                                                       int* live_moved, int* e_len, int* start_ind, const int* cur_t, int n_env, int cap) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * LV_WAVES + (threadIdx.x >> 6);  // (r is wave-uniform)
    if (r >= n) return;
    const int env = env_ids[r];
    if (env < 0 || env >= n_env) return;  // (no read or write goes through an index outside the batch)
    if (restart && restart[r]) return;
    // no index read from memory reaches the bank unchecked: len in 0 .. cap, S in 0 .. len - 1
    const int len = min(max(live_len[env], 0), cap), si = start_ind[env];
    const int S = min(max(uhc_lw_discard(len, cap, si, cur_t[env]), 0), len - 1);
    if (S < 1) return;
    double2* slice = reinterpret_cast<double2*>(bank + (size_t)env * cap * UHC_FRAME_STRIDE);
    // Records S .. len - 1 go to slots 0 .. len - 1 - S; when S < len - S the two ranges overlap.  No barrier is needed: every lane moves the SAME columns
    // (lane, lane + 64, ...) of every record, in ASCENDING record order.  Column j of slot d is written when record d + S is moved and read when record d is
    // moved (if d >= S) -- by the same lane, and d < d + S, so the read lies earlier in that lane's program order; no other lane touches the column.
    const bool tail = lane + 256 < LV_REC16;
    for (int k = S; k < len; k++) {
        const double2* src = slice + (size_t)k * LV_REC16;
        double2* dst = slice + (size_t)(k - S) * LV_REC16;
        // (named values, not an array: a conditionally written private array is placed in LDS by the compiler; the five loads are in flight together)
        const double2 v0 = src[lane], v1 = src[lane + 64], v2 = src[lane + 128], v3 = src[lane + 192];
        const double2 v4 = tail ? src[lane + 256] : v3;
        dst[lane] = v0, dst[lane + 64] = v1, dst[lane + 128] = v2, dst[lane + 192] = v3;
        if (tail) dst[lane + 256] = v4;
    }
    if (lane == 0) {  // (values computed from what was read above, not read again: an env listed twice cannot run a counter out of its range)
        live_len[env] = len - S;
        e_len[env] = len - S;
        start_ind[env] = si - S;
        live_base[env] += S;
        live_moved[env] += len - S;
    }
}

// E's per-env arrays and the live state -> one launch on s (two while sliding: the slide of the listed envs, then the append); n >= 1
extern "C" hipError_t uhc_launch_live_push(const EnvArgs* E, const LiveState* L, const int* env_ids, int n, const double* qpos, const double* root_record,
                                           const int* restart, const int* model, hipStream_t s) {
    if (L->slide) {
        hipLaunchKernelGGL(uhc_live_slide_kernel, dim3((unsigned)(((long long)n + LV_WAVES - 1) / LV_WAVES)), dim3(64 * LV_WAVES), 0, s, env_ids, restart, n, L->bank,
                           L->len, L->base, L->moved, E->e_len, E->start_ind, E->cur_t, E->n_env, L->cap);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    LiveArgs A = {};
    A.env_ids = env_ids, A.qpos = qpos, A.root_record = root_record, A.restart = restart, A.model = model, A.n = n;
    A.bank = L->bank, A.prev_qpos = L->prev_qpos, A.live_len = L->len, A.dropped = L->dropped, A.live_base = L->base, A.live_moved = L->moved;
    A.body_pos = L->body_pos, A.body_ipos = L->body_ipos;
    A.n_env = E->n_env, A.cap = L->cap, A.n_models = L->models, A.dt = L->dt, A.tree = L->tree;
    A.e_len = E->e_len, A.e_start = E->e_start, A.clip_id = E->clip_id, A.env_model = E->env_model, A.height_lb = E->height_lb;
    hipLaunchKernelGGL(uhc_live_push_kernel, dim3((unsigned)(((long long)n + 2 * LV_WAVES - 1) / (2 * LV_WAVES))), dim3(64 * LV_WAVES), 0, s, A);
    return hipGetLastError();
}
