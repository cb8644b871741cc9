// uhc_host.h -- the host-side objects behind the C-ABI's opaque handles, shared by uhc_capi.cpp (device work) and uhc_plan.cpp (planning).  Private to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/uhc_amd.h"
#include "uhc_device.h"

// ------------------------------------------------------------------ model (host copy)
struct UhcModel {
    UhcModelDesc d;  // scalars; pointers re-targeted at the vectors below
    std::vector<int32_t> body_parentid, body_jntadr, body_jntnum, body_dofadr, body_dofnum;
    std::vector<double> body_pos, body_quat, body_ipos, body_iquat, body_mass, body_inertia, body_invweight0;
    std::vector<int32_t> jnt_type, jnt_bodyid, jnt_qposadr, jnt_dofadr, jnt_limited;
    std::vector<double> jnt_pos, jnt_axis, jnt_range, jnt_stiffness, jnt_margin, qpos0, qpos_spring;
    std::vector<int32_t> dof_bodyid, dof_jntid, dof_parentid, dof_madr;
    std::vector<double> dof_armature, dof_damping, dof_frictionloss, dof_invweight0;
    std::vector<int32_t> geom_type, geom_bodyid, geom_contype, geom_conaffinity, geom_condim, geom_vertadr, geom_vertnum;
    std::vector<double> geom_pos, geom_quat, geom_size, geom_friction, geom_margin, geom_gap, geom_solref, geom_solimp,
        geom_rbound, geom_center, mesh_vert;
    std::vector<int32_t> mesh_adjadr, mesh_adj, exclude_pair, actuator_dofid;
    std::vector<double> actuator_gear;
};

// ------------------------------------------------------------------ batch
// the caps on the sticky tiers' consumer launches (UHC_Q* knobs: read_knobs -> the batch -> plan_sticky_step)
struct QueueCaps {
    int q2_div = 1;        // waiting general-tier consumers per expected env: 1 / q2_div (UHC_Q2_DIV >= 1)
    int q2_wait_min = 16;  // at least so many general-tier consumers wait for hand-ons (UHC_Q2_WAIT >= 1)
    int q2_max = 256;      // most general-tier consumers beside a fast tier that still has most of the envs (UHC_Q2_MAX >= 16)
    int q3_max = 32;       // most large-tier consumers in that regime (UHC_Q3_MAX >= 2)
    int q4_max = 16;       // most tier-4 consumers (UHC_Q4_MAX >= 0; 0: none -- what the large tier hands on waits for the chained launch at the end of the step)
};
// the per-step words of a batch: seven int arrays in ONE allocation that starts at DevState::redo (the step's UHC_F_REDO words) and that launch() clears with
// one memset per step.  Offsets in ints from redo; ticket is one word, the others have one per env.
struct StepWords { size_t pend2, pend3, resume, why, chunk_done, ticket, total; };
inline StepWords step_words(size_t n_env) { return {n_env, 2 * n_env, 3 * n_env, 4 * n_env, 5 * n_env, 6 * n_env, 6 * n_env + 1}; }

struct UhcBatch {
    int n_env = 0, device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    KernelArgs A;
    size_t lds_bytes = 0, lds_bytes_fast = 0, lds_bytes_big = 0;
    bool use_fast = true;
    bool general_only = false;
    // uhc_batch_set_kernel_path(2): sticky tiers -- every env starts a step in the tier that computed its last one (DevState::tier)
    int path_mode = 0;
    hipStream_t side_stream = nullptr, side_stream3 = nullptr, side_stream4 = nullptr;  // kernel path 2: the general / large tiers' own envs run beside the fast tier's
    hipEvent_t ev_fork = nullptr, ev_side1 = nullptr, ev_side2 = nullptr, ev_side3 = nullptr;
    int* tier_now = nullptr;
    bool large_first = false;  // the large tier's consumers are launched (and resident) before the general tier's
    int n_cu = 256;
    std::vector<std::pair<char*, size_t>> fences;  // UHC_GUARD_LDS=1: (base, payload bytes) of every fenced device array
    int* d_guard_hits = nullptr;  // UHC_GUARD_LDS=1: the kernels' report (KernelArgs::guard_hits), printed by uhc_batch_sync / uhc_batch_free
    int guard_reported = 0;
    int* d_order = nullptr;  // launch order of the fast tier under sticky tiers (uhc_tier_lists_kernel)
    int aborts_seen = 0, abort_events = 0;
    long long queues_off_until = 0;
    QueueCaps caps;
    int fast_chunk = 0;      // substeps per chunk of the fast tier's control step (UHC_FAST_CHUNK; 0: default_fast_chunk decides)
    int *d_lists = nullptr, *d_counts = nullptr, *d_cursors = nullptr, *d_fin = nullptr;  // the queues' words: UhcList / UhcCount / UhcCursor / UhcFin (uhc_device.h)
    bool queues_off = false;
    int* h_counts = nullptr;  // pinned [8][UHC_N_WORDS]: d_counts as the last eight steps left it (rows indexed by UhcCount), copied back asynchronously
    hipEvent_t cnt_ev[8] = {};
    long long cnt_step = 0;
    std::vector<void*> allocs;
    int nM = 0;
    int* reset_mask = nullptr;
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_used, ev_free;
    int n_models = 1;
    int n_trailing_free = 0;  // free bodies at the end of the model (objects)
    bool hbm_guard = false;  // UHC_GUARD_LDS=1 / 2: zero-initialised device arrays sit between fences (dalloc)
    struct Field { void* ptr; int64_t count; };
    Field field[UHC_F_COST + 1] = {};  // uhc_batch_field: UHC_F_* -> (device pointer, elements)
};
