// uhc_plan.h -- what uhc_batch_create decides before it touches the device: knobs, topology tables, LDS layouts, schedules, launch sizes.
// Pure host code (uhc_plan.cpp calls no hip* function); tests/test_batch_plan_cpu.py checks it without a GPU.
#pragma once
#include <string>
#include <vector>

#include "uhc_host.h"
#include "uhc_step_words.h"

// the UHC_* environment variables of batch creation, parsed and range-checked (read_knobs is the one place of the host code that reads the environment)
struct BatchKnobs : QueueCaps {    // (the caps: UHC_Q2_DIV, UHC_Q2_WAIT, UHC_Q2_MAX, UHC_Q3_MAX, UHC_Q4_MAX)
    int dbg = 0;                    // UHC_DEBUG (KernelArgs::dbg: enum UhcDebug; UHC_DEBUG_EXP_* only in -DUHC_EXPERIMENTS builds)
    int marks[UHC_N_MARKS] = {64, 16, -1, 56, 14, 10, 8, 7};  // UHC_TIER_MARKS "a,b,c,d,e,f,g,h" in UhcMark's order (the body-body up mark < 0: the body-body marks follow the fast layout)
    int fast_dense_got = 0, fast_dense_kib = 0, fast_dense_rows = 0, fast_dense_con = 0;  // UHC_FAST_DENSE "KiB,dense rows[,contacts]": fields read, their values
    bool fast_dcol_own = false;     // UHC_FAST_DCOL_OWN=1
    bool lds_pad_fast = false;      // UHC_LDS_PAD_FAST=KiB
    int lds_pad_fast_kib = 0;
    bool force_general = false;     // UHC_FORCE_GENERAL=1
    int tiers = 0;                  // UHC_TIERS: 2, 3 or 0 (unset / anything else: four tiers)
    int guard = 0;                  // UHC_GUARD_LDS: 1 guard words, 2 the self-test (one guard ON qpos of the fast tier), 0 off
    int t4_rows = 0;                // UHC_T4_ROWS >= 0
    int fast_chunk = 0;             // UHC_FAST_CHUNK=<substeps>: the fast tier's control step runs in chunks of so many substeps (0: not given, default_fast_chunk
                                    // decides; a value >= n_substeps, and "0" itself, mean one chunk: the whole-step launch)
    bool fast_chunk_bad = false;    // ... was given and is not a non-negative integer: plan_batch refuses the batch
};
BatchKnobs read_knobs();

struct BatchPlan {
    KernelArgs A;  // every pointer-free field batch creation decides; the pointers are null (uhc_batch_create uploads the tables below)
    size_t lds_bytes = 0, lds_bytes_fast = 0, lds_bytes_big = 0;
    bool use_fast = true;
    int n_trailing_free = 0;
    std::vector<int> body_depth, body_rootid, body_nsub, body_lastdof, dof_depth, dof_ndesc, dof_rootid;
    std::vector<short> dof_anc, m_row, m_col;
    std::vector<unsigned short> m_ij;
    std::vector<unsigned char> ncommon;
    std::vector<unsigned long long> chainmask;  // [nv][2] bit d: dof d is on the chain of dof i (DevTopo::dof_chainmask)
    std::vector<int> pg1, pg2, cg1, cg2;  // statically filtered collision pairs: (plane, hull), (hull, hull)
    std::vector<double> model_blob;       // the models' numeric blobs, one after the other (DevNumOff::stride each)
    std::vector<unsigned int> fac_prog, sol_back, sol_fwd, chain;
    std::vector<int> dof_act;
    std::vector<int> vf_body;    // explicit RFC only
    std::vector<int> guard_tab;  // UHC_GUARD_LDS: 4 x 64 ints (KernelArgs::guard_tab); empty otherwise
};
// -> 0, or 1 with *err set: every refusal of uhc_batch_create that does not need the device
int plan_batch(const UhcModel* const* models, int n_models, const int32_t* env_model, int n_env, const UhcCtrlDesc* ctrl, const BatchKnobs& knobs,
               BatchPlan* out, std::string* err);

// ------------------------------------------------------------------ sticky tiers: one step's launches from the newest queue counts the host has seen
// (launch_sticky() in uhc_capi.cpp calls these three in turn: sticky_launch4, plan_sticky_step, sticky_wiring)

// Do tier 4's queue consumers run this step?  The list kernel needs the answer at the head of the step (it fills their queue), before the host waits for
// older counts and updates its back-off: queues_off here is the value the step BEGINS with.  est4, est2_then: as in StickyInputs
bool sticky_launch4(int last_tier, int est4, int est2_then, bool queues_off);
struct StickyInputs {
    int est2, est3, est4;  // queue lengths of the general / large tier at the end of the newest step seen; env-steps that went through tier 4
    int est2_then;         // the general tier's queue in the step est4 is from
    int handed2;           // how many of est2 came in during the step
    int n_env, n_cu;
    size_t lds_bytes_fast;
    bool large_first;      // the large tier's consumers are launched before the general tier's
    int last_tier;
    bool queues_off;       // no waiting consumers (back-off after a consumer gave up)
    int q2_div, q2_wait_min, q2_max, q3_max, q4_max;  // QueueCaps, member for member (set_caps): the test probes fill this struct by position AND set these by name
    bool fixed_cap2;       // measurement switch (UHC_DEBUG_EXP_FIXED_CAP2 of -DUHC_EXPERIMENTS builds): a fixed cap UHC_Q2_MAX on the general tier's consumers
    int fast_chunk;        // BatchKnobs::fast_chunk (0: the default), and the control step's substeps (0: the fast tier's launch is not chunked)
    int n_substeps;
};
// the fast tier's launch in substep chunks (uhc_step_kernel<0, 1, *>): chunk c of an env runs the substeps [c chunk, min((c + 1) chunk, n_substeps))
struct FastChunks {
    int chunk;       // substeps per chunk; 0: one workgroup per env runs the whole step (KernelArgs::chunk)
    int n_chunks;
    int grid;        // workgroups of the launch: n_chunks x n_env
    int prod_total;  // what the general tier's consumers wait for: every workgroup of the launch
};
FastChunks plan_fast_chunks(int n_substeps, int chunk, int n_env);  // chunk <= 0 or >= n_substeps: one chunk
void fast_chunk_range(const FastChunks& f, int n_substeps, int c, int* lo, int* hi);
// the chunk size of a launch: the knob when given, else by whether the batch fills the chip's places for fast-tier workgroups more than once
int default_fast_chunk(int knob, int n_substeps, int n_env, int n_cu, size_t lds_bytes_fast);
struct StickySizes {
    bool queues, waiting, q3, q4, launch4;  // consumers of the general tier / ... that wait for the fast tier's hand-ons / of the large tier / of tier 4; the launch4 given
    int grid2, grid3, grid4, n_wait, sticky_mask;  // (sticky_mask: KernelArgs::sticky_mask of the step's side launches and of the fast tier's)
    FastChunks fast;
};
inline void set_caps(StickyInputs& in, const QueueCaps& c) { in.q2_div = c.q2_div; in.q2_wait_min = c.q2_wait_min; in.q2_max = c.q2_max; in.q3_max = c.q3_max; in.q4_max = c.q4_max; }
// launch4: sticky_launch4 as the step's list kernel was told; the library calls this once per step.  The form without it is the step in which the back-off does
// not flip -- in.queues_off decides both --, which is what the recorded sticky cases of tests/batch_plan_recording.json are
StickySizes plan_sticky_step(const StickyInputs& in, bool launch4);
inline StickySizes plan_sticky_step(const StickyInputs& in) { return plan_sticky_step(in, sticky_launch4(in.last_tier, in.est4, in.est2_then, in.queues_off)); }

// The step's launches beside each other as a table: who consumes which queue, whose exits a consumer waits for, who hands on to whom, which gate holds which
// launch back.  Slots are indices into the batch's lists / counts / cursors / fin (UhcList / UhcCount / UhcCursor / UhcFin, uhc_device.h); UHC_NONE: the launch
// does not use the field (a null pointer or 0 in its KernelArgs).  The chained launches that follow on the batch's stream use none of this and are not listed.
#define UHC_NONE (-1)
enum StepStream { STREAM_MAIN = 0, STREAM_GEN = 1, STREAM_BIG = 2, STREAM_T4 = 3 };  // the batch's stream and the side streams of the general / large tier / tier 4
struct StepLaunch {
    int tier;                        // 4, 3, 2: queue consumers of that tier; 1: the fast tier's launch, one workgroup per (chunk, env)
    int stream;                      // StepStream
    int list, count, cursor;         // the queue this launch consumes
    int grid;                        // workgroups
    int n_wait, spares;              // so many workgroups that find the queue empty stay and wait; the counter of the seats taken (none: every one may wait)
    int started;                     // bumped once per workgroup on entry
    int prod_fin, prod_total;        // the queue's producers: it can grow until this counter has reached prod_total (none: it does not grow)
    int fin;                         // bumped once per workgroup on exit
    int next_list, next_count;       // where an env this tier cannot hold is handed on (none: it is flagged for the chained launches)
    int gate_started, gate_want;     // a gate in front of the launch, on its stream: until so many workgroups have bumped that counter (none: no gate)
    int gate_waited;                 // ... the count slot that receives the gate's wait
    int tier_want, chunk;            // the fast tier's: KernelArgs::tier_want, substeps per chunk (0: the whole step)
    bool use_order;                  // ... and it runs in the list kernel's launch order
};
struct StepWiring { int n; StepLaunch launch[4]; };  // in launch order: tier 4, then large before general exactly when large_first, the fast tier last
StepWiring sticky_wiring(const StickySizes& z, bool large_first);
