// uhc_step_words.h -- the device half of the sticky tiers' control plane as plain integer code: the words a step reports about itself (the forward pass's
// status word, UHC_F_REDO, UHC_F_HANDON_WHY, the chunk record) and the policy that reads them (the tier an env starts its next step in, the fast tier's
// launch order).  No lanes, no LDS, no HIP runtime call: the kernels inline these functions, tests/test_step_words_cpu.py compiles them with the host
// compiler.  The public words' bits are include/uhc_amd.h's (UHC_REDO_*, UHC_HANDON_*).
#pragma once
#include "../../include/uhc_amd.h"  // (the public bits of UHC_F_REDO and UHC_F_HANDON_WHY: UHC_REDO_*, UHC_HANDON_*)
#include "uhc_device.h"

// (force-inlined, i.e. before anything is optimised, and scalars in and out: what keeps the kernels' code closest to the one these expressions gave while they stood
//  in uhc_step_env -- an aggregate or a by-reference local there changes the order in which the compiler promotes ALL its locals to registers; profiles/step_words_isa.txt)
#define UHC_WORDS_FN __host__ __device__ __forceinline__


// ------------------------------------------------------------------ the forward pass's status word (FwdOut::overflow, OR-ed over the substeps of a step)
enum UhcStatus : int {
    UHC_ST_HANDON = 1,          // the env does not fit this tier: nothing is committed, the next tier redoes it (only raised by a tier that hands on)
    UHC_ST_DROPPED = 2,         // rows / contacts beyond the capacity were dropped (the last tier; the fast tier in truncate mode)
    UHC_ST_SWEPT = 4,           // solved by sweeps to tolerance (solver 1: the working sets gave up; with tier 4 only for friction-loss rows)
    UHC_ST_WHY_FRICTION = 8,    // ... because the env has friction-loss rows (box constraints)
    UHC_ST_WINDOWED = 16,       // an island was solved in windows of 64 rows: not a fallback
    UHC_ST_WHY_NOCONV = 32,     // ... because the working-set rounds did not converge
    UHC_ST_WHY_PIVOT = 64,      // ... because the pivoting broke down / did not converge on a working set
    UHC_ST_PRIMAL = 128,        // solved by Newton on the primal (tier 4)
    UHC_ST_PRIMAL_CAP = 256     // ... and that iteration stopped at its cap (the best iterate is used)
};
// why a tier could not hold an env (bits 16+ of the status word; UHC_F_HANDON_WHY holds the byte of the env's last hand-on per tier)
#define UHC_WHY_SHIFT 16
#define UHC_WHY_CONTACTS (UHC_HANDON_CONTACTS << UHC_WHY_SHIFT)
#define UHC_WHY_ROWS (UHC_HANDON_ROWS << UHC_WHY_SHIFT)
#define UHC_WHY_DENSE_SLOTS (UHC_HANDON_DENSE_SLOTS << UHC_WHY_SHIFT)
#define UHC_WHY_ROW_STORAGE (UHC_HANDON_ROW_STORAGE << UHC_WHY_SHIFT)
#define UHC_WHY_CANDIDATES (UHC_HANDON_CANDIDATES << UHC_WHY_SHIFT)
#define UHC_WHY_SOLVER (UHC_HANDON_SOLVER << UHC_WHY_SHIFT)  // the working sets of the general / large tier did not finish (more than 64 force-carrying rows in an island, no convergence): Newton on the primal takes over
static_assert(UHC_WHY_SOLVER == (1 << 21) && UHC_ST_PRIMAL_CAP < (1 << UHC_WHY_SHIFT), "the reasons of a hand-on sit above the status bits");

// k_as_general's return codes below zero (>= 0: the rounds it took, | UHC_WS_WINDOWED)
enum UhcWsGaveUp {
    UHC_WS_FRICTION = -1,  // friction-loss rows: the sweeps' business
    UHC_WS_LOST = -2,      // a pass that dropped rows met an island that needs windows: not worth them (k_forward), and no reason bit
    UHC_WS_NOCONV = -3,    // the rounds ended without every island done
    UHC_WS_PIVOT = -4,     // pivot breakdown / no convergence of the pivoting on a working set
    UHC_WS_TIER4 = -5      // an island with more force-carrying rows than lanes, and tier 4 behind this one: the env is handed on, never swept
};
// Why the working sets gave up, as a status bit beside UHC_ST_SWEPT.  The reason bits are laid out so that a code with a reason shifts the swept bit onto it:
// the asserts below are the mapping, code by code.  UHC_WS_LOST has no reason -- its place is the windowed bit's -- and k_forward leaves it out by name; the
// sweeps of solver 0 are no fallback at all.  (Text and a shift, not a function: as two inlined calls this line took the large tier's forward-only kernel from 1047 to 1045 SGPR spills and
// 231 instructions up; as it stands every step kernel keeps the parent's registers, spills and scratch -- profiles/step_words_isa.txt.)
#define UHC_WS_REASON(code) (UHC_ST_SWEPT << (-(code)))
static_assert(UHC_ST_SWEPT << -UHC_WS_FRICTION == UHC_ST_WHY_FRICTION && UHC_ST_SWEPT << -UHC_WS_NOCONV == UHC_ST_WHY_NOCONV && UHC_ST_SWEPT << -UHC_WS_PIVOT == UHC_ST_WHY_PIVOT,
              "code -> reason bit");
static_assert(UHC_ST_SWEPT << -UHC_WS_LOST == UHC_ST_WINDOWED, "the one code between them would land on the windowed bit: k_forward leaves it out");
static_assert(UHC_ST_WHY_FRICTION != UHC_ST_WINDOWED && UHC_ST_WHY_NOCONV != UHC_ST_WINDOWED && UHC_ST_WHY_PIVOT != UHC_ST_WINDOWED, "no reason bit is the windowed bit");
// (UHC_WS_TIER4 never gets here: only a tier with tier 4 behind it returns it, and that tier hands the env on)

// ------------------------------------------------------------------ UHC_F_REDO
// status bit -> public bit: the reasons and the windowed bit lie one place lower in UHC_F_REDO
#define UHC_REDO_SHIFTED (UHC_REDO_WHY_FRICTION | UHC_REDO_WINDOWED | UHC_REDO_WHY_NOCONV | UHC_REDO_WHY_PIVOT)
static_assert((UHC_ST_WHY_FRICTION >> 1) == UHC_REDO_WHY_FRICTION && (UHC_ST_WINDOWED >> 1) == UHC_REDO_WINDOWED && (UHC_ST_WHY_NOCONV >> 1) == UHC_REDO_WHY_NOCONV &&
              (UHC_ST_WHY_PIVOT >> 1) == UHC_REDO_WHY_PIVOT && UHC_REDO_SHIFTED == 0x3c, "redo_word moves these four with one shift");
// the step's swept mask after substep `it` ended with `status` (the forward pass of a restart, it < 0, and a substep beyond the field have no bit)
UHC_WORDS_FN int redo_swept_mask(int mask, const int status, const int it) {
    if ((status & UHC_ST_SWEPT) && it >= 0 && it < UHC_REDO_SWEPT_SUBSTEPS) mask |= UHC_REDO_SWEPT_SUBSTEP0 << it;
    return mask;
}
static_assert((long long)UHC_REDO_SWEPT_SUBSTEP0 << UHC_REDO_SWEPT_SUBSTEPS == UHC_REDO_PRIMAL_CAP, "the substep bits end below the primal solver's two");
// Does a step of `tier` that was not handed on write UHC_F_REDO?  The fast tier leaves the step's cleared word unless it dropped rows (truncate mode)
UHC_WORDS_FN bool redo_written(const int tier, const int status) { return tier != 1 || (status & UHC_ST_DROPPED) != 0; }
// ... and the word it writes
UHC_WORDS_FN int redo_word(const int tier, const int status, const int swept_mask) {
    if (tier == 1) return (status & UHC_ST_DROPPED) ? UHC_REDO_DROPPED : 0;
    return UHC_REDO_GENERAL | ((status & UHC_ST_SWEPT) ? UHC_REDO_SWEPT : 0) | ((status >> 1) & UHC_REDO_SHIFTED) | (tier >= 3 ? UHC_REDO_LARGE : 0) |
           ((status & UHC_ST_DROPPED) ? UHC_REDO_DROPPED : 0) | swept_mask | ((status & UHC_ST_PRIMAL) ? UHC_REDO_PRIMAL : 0) | ((status & UHC_ST_PRIMAL_CAP) ? UHC_REDO_PRIMAL_CAP : 0);
}

// ------------------------------------------------------------------ UHC_F_HANDON_WHY
// the word after tier `tier` handed the env on in substep `substep`: the fast / general tier replace their own byte and the substep, the large tier adds its byte
UHC_WORDS_FN int handon_why_word(const int tier, const int old_word, const int status, const int substep) {
    const int why = (status >> UHC_WHY_SHIFT) & UHC_HANDON_FIELD;
    if (tier <= 2)
        return (old_word & (tier == 1 ? UHC_HANDON_FIELD << UHC_HANDON_GENERAL_SHIFT : UHC_HANDON_FIELD << UHC_HANDON_FAST_SHIFT)) |
               (why << (tier == 1 ? UHC_HANDON_FAST_SHIFT : UHC_HANDON_GENERAL_SHIFT)) | ((substep & UHC_HANDON_FIELD) << UHC_HANDON_SUBSTEP_SHIFT);
    return old_word | why << UHC_HANDON_LARGE_SHIFT;
}

// ------------------------------------------------------------------ the chunk record (KernelArgs::chunk_rec, UHC_CHUNK_REC ints per env)
enum UhcChunkRecWord {
    UHC_REC_PK_NEFC = 0, UHC_REC_PK_NCON = 1, UHC_REC_PK_NTWO = 2, UHC_REC_PK_Y = 3, UHC_REC_PK_ACT = 4,  // the peaks of the step's substeps so far: they decide the env's next tier and its place in the launch order
    UHC_REC_NCON = 5, UHC_REC_NEFC = 6, UHC_REC_ITERS = 7,  // ncon / nefc / solver_iter of the step's newest forward pass
    UHC_REC_STATUS = 8,                                     // the status word so far (the fast tier's: the truncation bit)
    UHC_REC_WORDS = 9
};
static_assert(UHC_REC_WORDS <= UHC_CHUNK_REC, "the record fits its allocation");
UHC_WORDS_FN int step_imax(const int a, const int b) { return a > b ? a : b; }
// One word of the earlier chunks' record merged into this chunk's: a peak by maximum, the status by OR (the counts of the newest forward pass are not merged).
UHC_WORDS_FN int chunk_rec_merged(const int word, const int mine, const int earlier) { return word == UHC_REC_STATUS ? (mine | earlier) : step_imax(mine, earlier); }

// ------------------------------------------------------------------ KernelArgs::marks (UHC_TIER_MARKS "a,b,c,d,e,f,g,h" in this order)
enum UhcMark {
    UHC_MARK_UP2_ROWS = 0, UHC_MARK_UP2_CON = 1, UHC_MARK_UP2_TWO = 2,  // fast -> general above so many rows / contacts / body-body rows (of 64 / 16 / 12)
    UHC_MARK_DN1_ROWS = 3, UHC_MARK_DN1_CON = 4, UHC_MARK_DN1_TWO = 5,  // ... and down to the fast tier again at or below these
    UHC_MARK_UP3_8THS = 6,                                              // general -> large above so many eighths of any of the general tier's capacities
    UHC_MARK_DN2_8THS = 7,                                              // large -> general at or below so many eighths of all of them
    UHC_N_MARKS = 8
};
static_assert(sizeof(KernelArgs::marks) == UHC_N_MARKS * sizeof(int), "one mark per name");

// ------------------------------------------------------------------ where the env's next step starts (uhc_batch_set_kernel_path 2)
// An env comes down a tier only with room to spare.
// An env that comes CLOSE to a tier's capacity starts its next step one tier up: finding out in the middle of a step that it no
// longer fits costs that tier's work so far, and the step then ends a whole general- (or large-) tier env-step after the moment
// of the hand-on -- with a thousand envs some env does that every step, and every step lasts fast + general + large.  It comes
// down again only well below the mark (hysteresis).  The marks are the batch's (KernelArgs::marks, UHC_TIER_MARKS).
// tier: the tier that finished the step; pk_*: the step's peaks over its substeps -- rows, contacts, body-body rows, packed Yhat entries, force-carrying rows.  sticky4: the measurement switch UHC_DEBUG_EXP_STICKY_TIER4 (read by the kernel, behind UHC_EXP)
UHC_WORDS_FN int next_tier(const int tier, const int pk_nefc, const int pk_ncon, const int pk_ntwo, const int pk_y, const int pk_act, const KernelArgs& A, const bool sticky4) {
    const int* mk = A.marks;  // up2: rows, contacts, body-body rows | dn1: the same | up3, dn2: eighths of the general tier's capacities
    const bool up2 = pk_nefc > mk[UHC_MARK_UP2_ROWS] || pk_ncon > mk[UHC_MARK_UP2_CON] || pk_ntwo > mk[UHC_MARK_UP2_TWO];   // of 64 rows / 16 contacts / 12 body-body rows
    // (... and only if its packed rows fit the fast tier's storage: with objects in the model that storage is small, and an env that
    //  fits by rows and contacts alone came down every step only to be handed on in its first forward pass)
    const bool dn1 = pk_nefc <= mk[UHC_MARK_DN1_ROWS] && pk_ncon <= mk[UHC_MARK_DN1_CON] && pk_ntwo <= mk[UHC_MARK_DN1_TWO] && (tier == 1 || pk_y + 8 <= (7 * A.cf.ycap) / 8);
    const bool up3 = pk_nefc > (mk[UHC_MARK_UP3_8THS] * A.cg.maxefc) / 8 || pk_ncon > (mk[UHC_MARK_UP3_8THS] * A.cg.maxcon) / 8 || pk_ntwo > (mk[UHC_MARK_UP3_8THS] * A.cg.ndense) / 8 ||
                     pk_y > (mk[UHC_MARK_UP3_8THS] * A.cg.ycap) / 8;
    const bool dn2 = pk_nefc <= (mk[UHC_MARK_DN2_8THS] * A.cg.maxefc) / 8 && pk_ncon <= (mk[UHC_MARK_DN2_8THS] * A.cg.maxcon) / 8 && pk_ntwo <= (mk[UHC_MARK_DN2_8THS] * A.cg.ndense) / 8 &&
                     pk_y <= (mk[UHC_MARK_DN2_8THS] * A.cg.ycap) / 8;
    const int big = A.last_tier >= 3 ? 3 : 2;
    int next;
    if (tier == 1) next = up2 ? 2 : 1;
    else if (tier == 2) next = (up3 && big == 3) ? 3 : (dn1 ? 1 : 2);
    else next = !dn2 ? 3 : (dn1 ? 1 : 2);
    // an env that needed tier 4 (beyond the large tier's capacities, or more force-carrying rows than its working sets finish) starts its next
    // step THERE: at the head of the queue of tier 4's consumers (uhc_capi.cpp) instead of an abandoned large-tier attempt first.  It comes down with room to spare: 3/4 of the large tier's capacities and <= 48 rows with a force.
    // OPT-IN (UHC_DEBUG_EXP_STICKY_TIER4): measured on the random-policy ball-joint rollouts it LOSES -- configs[4] 41.6 k -> 27.1 k env-steps/s: the envs that
    // reach tier 4 there are diverging ones that reset within two or three steps, a reset env then runs its first step in tier 4 too, and a whole step of
    // primal solves costs more than the large-tier attempt it saves -- so by default such an env starts its next step in the large tier.
    // Heavy envs go STRAIGHT to tier 4 (round 6): the four-wave Newton iteration on the primal costs the same whatever the number of rows, while a
    // general- or large-tier env-step grows with every working-set round -- and the step's slowest env is what a control step waits for.  An env
    // whose step peaked at KernelArgs::t4_rows rows or more starts its next step at the head of tier 4's queue and stays while it peaks above 3/4 of that.
    if (A.last_tier == 4 && A.t4_rows > 0 && ((tier == 2 || tier == 3) ? pk_nefc >= A.t4_rows : (tier == 4 && 4 * pk_nefc >= 3 * A.t4_rows))) next = 4;
    // (Sending SLOW envs there too -- by the duration of their last general-tier step -- was built and measured in round 6 and is gone again: a tier-4 env-step of a
    //  60-80-row env is no shorter than its general-tier one, and a whole CU per env is what the fast tier's second round needs: profiles/r06_q_t4ticks_sweep.txt.)
    if (tier == 4 && sticky4 && A.last_tier == 4 && !(pk_nefc <= (3 * A.ch.maxefc) / 4 && pk_ncon <= (3 * A.ch.maxcon) / 4 && pk_ntwo <= (3 * A.ch.ndense) / 4 && pk_act <= 48)) next = 4;
    return next;
}

// ------------------------------------------------------------------ the fast tier's launch order
// UHC_F_COST: how close the step came to ANY of the fast tier's capacities, in sixty-fourths -- rows, contacts,
// body-body rows and (round 6) the packed row storage, which names 2 of 3 hand-ons of the ball-joint rollouts (tools/tier_trace.py) -- and at the top of
// the scale an env whose joints spin faster than any tracked motion's: a simulation on its way to the bad-value flag piles up rows within a few
// substeps, goes through every tier and ends the step if it starts in the launch's last round (profiles/r06_b_tier_trace_configs4.txt)
// vmax_end: the largest |qvel| at the end of the step
UHC_WORDS_FN int launch_cost(const int pk_nefc, const int pk_ncon, const int pk_ntwo, const int pk_y, const double vmax_end, const KernelArgs& A) {
    int cost = step_imax(pk_nefc, step_imax((pk_ncon * UHC_FAST_MAXEFC) / step_imax(A.cf.maxcon, 1), (pk_ntwo * UHC_FAST_MAXEFC) / step_imax(A.cf.ndense, 1)));
    cost = step_imax(cost, (int)(((long long)pk_y * UHC_FAST_MAXEFC) / step_imax(A.cf.ycap, 1)));
    if (vmax_end > 60.0) cost = step_imax(cost, UHC_FAST_MAXEFC); else if (vmax_end > 30.0) cost = step_imax(cost, 40);
    return cost;
}
// The list kernel's buckets (uhc_tier_lists_kernel): the fast tier's envs from the costliest bucket down, then the envs that are not this launch's.
#define UHC_ORDER_BUCKETS 9
// The batch's per-env words -- tier: where the env's last step left it (DevState::tier); masked, active: the step has a mask, and the mask; fresh; cost: UHC_F_COST,
// 0 .. 64+ -- as arrays, so that the kernel reads only the words the answer depends on
// (Arrays and an index here and in start_tier, and start_tier's second rule on its own, instead of four ints: that is the form in which uhc_tier_lists_kernel
//  stays instruction for instruction what it was -- an int argument is a load the kernel did not make; the probe of tests/test_step_words_cpu.py puts them together as the kernel does.)
UHC_WORDS_FN int order_bucket(const int* tier, const bool masked, const int* active, const int* fresh, const int* cost, const int env) {
    if (tier[env] != 1 || (masked && !active[env])) return UHC_ORDER_BUCKETS;
    // (an env restarted since its last step has no history: its reset pose may not fit the tier at all -- many do not -- and it is handed
    //  on in its first forward pass; at the head of the launch that happens while the next tier's consumers still have the step ahead)
    if (fresh[env]) return 0;  // (a bucket of their own, ahead of everything: with the row storage in the cost, the next bucket holds hundreds of envs)
    // (round 6: the cost counts the packed row storage too, which on the ball-joint / object models puts most envs within an eighth of the capacity:
    //  the scale is fine where the hand-ons are -- an env that no longer fits in its first forward pass must not start in the launch's last round)
    const int c = cost[env];  // 0 .. 64+ (sixty-fourths of the capacity)
    return c >= 62 ? 1 : c >= 59 ? 2 : c >= 56 ? 3 : c >= 52 ? 4 : c >= 48 ? 5 : c >= 40 ? 6 : c >= 24 ? 7 : 8;
}
// The tier the step's launches find the env in (DevState::tier_now), in two rules.  A restarted env does not start in tier 4: it has no history, its reset pose
// is the general tier's to look at, not a whole CU's.  tier: where the env's last step left it; fresh: the batch's per-env words, read for a tier-4 env only
UHC_WORDS_FN int start_tier(int tier, const int* fresh, const int env) {
    if (tier == 4 && fresh[env]) tier = 2;
    return tier;
}
// ... and a tier-4 env is tier 4's only in a step whose tier-4 queue consumers run (launch4); without them it is the large tier's like any tier-3 env
UHC_WORDS_FN int start_tier4(const bool launch4) { return launch4 ? 4 : 3; }
