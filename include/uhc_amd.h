/*
 * uhc_amd.h -- C-ABI of libuhc_amd.so: batched SMPL-humanoid rigid-body simulation on MI355X.
 *
 * This is the drop-in boundary for the hot path named in BASELINE.json (north_star).  The
 * reference (ZhengyiLuo/UHC) reaches its physics through the mujoco-py object API; each entry
 * point below names the reference call site it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; uhc_last_error() gives the message
 *     (thread-local).  No exception crosses this boundary.  A physics blow-up is NOT an error: it
 *     raises the per-env `fail` flag, mirroring uhc/envs/humanoid_im.py:1207-1211.
 *   - handles are opaque; the library owns all device buffers it allocates.
 *   - `double* d_*` / `int* d_*` arguments are DEVICE pointers (HBM resident) unless the name
 *     starts with `h_`; all arrays are dense row-major, env-major ([n_env][dim]).
 *   - a UhcBatch is bound to one device and one HIP stream; calls on one batch are not
 *     re-entrant, different batches are independent (one per GPU / rank).
 *   - all arithmetic is float64, like the reference (scripts/train_uhc.py:80-81).
 */
#ifndef UHC_AMD_H
#define UHC_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: what this header declares is its whole export table */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define UHC_ABI_VERSION 11  /* 11: uhc_expert_frames (the clip bank's frame records computed on the device) -- uhc_eval_record / uhc_eval_metrics came later and are purely additive: still 11, as are uhc_surface_* / uhc_eval_record_pose and uhc_policy_*; 10: uhc_build_flags; 9: UHC_F_REDO bits 29 / 30 (tier 4), swept-substep bits 8 .. 28; uhc_rollout_record counts int64 [7] */

/* joint / geom type codes (MuJoCo numbering) */
enum { UHC_JNT_FREE = 0, UHC_JNT_BALL = 1, UHC_JNT_SLIDE = 2, UHC_JNT_HINGE = 3 };
enum { UHC_GEOM_PLANE = 0, UHC_GEOM_SPHERE = 2, UHC_GEOM_CAPSULE = 3, UHC_GEOM_BOX = 6, UHC_GEOM_MESH = 7 };
/* Geoms that collide: the plane against CONVEX HULLS, and hulls against each other (MPR).  A hull is a mesh geom or a ROUNDED hull: a sphere (one core vertex, its
 * centre) or a capsule (two core vertices, the ends of its segment: geom_pos +- half length along the geom's z axis, in that order), whose surface lies geom_size[0]
 * (the radius) beyond the core along the query direction -- [MJ-ext] mjc_PlaneSphere / mjc_PlaneCapsule for the plane, mjc_Convex's support callbacks for the rest.
 * The core vertices live in the mesh tables (geom_vertadr / geom_vertnum / mesh_vert / mesh_adj) like a mesh's hull vertices, in the BODY frame; boxes carry mass only. */

/*
 * Flat description of one compiled model (host arrays, copied by uhc_model_create).
 * Produced by uhc_amd/model/mjcf.py; replaces mujoco_py.load_model_from_xml
 * (uhc/khrylib/rl/envs/common/mujoco_env.py:18, uhc/envs/humanoid_im.py:1448).
 */
typedef struct UhcModelDesc {
    int32_t nq, nv, nu, nbody, njnt, ngeom, nmeshvert, nmeshadj, nexclude;
    int32_t iterations;        /* solver sweeps cap (MuJoCo opt.iterations, default 100) */
    int32_t plane_mesh_maxcon; /* max contacts a plane-mesh pair may emit */
    int32_t solver;            /* contact solve of the dual QP  min 1/2 f'Af + f'b, f >= 0:
                                * 0 = projected Gauss-Seidel sweeps up to `iterations` / `tolerance` ([MJ-ext] mj_solPGS);
                                * 1 = the same QP solved to its exact optimum by active-set iterations (block principal pivoting:
                                *     factor the free block, flip every infeasible row); envs with friction-loss rows use 0 */
    double timestep, tolerance, meaninertia;
    double gravity[3];
    /* bodies [nbody] */
    const int32_t *body_parentid, *body_jntadr, *body_jntnum, *body_dofadr, *body_dofnum;
    const double *body_pos /*[nbody][3]*/, *body_quat /*[nbody][4]*/, *body_ipos, *body_iquat;
    const double *body_mass, *body_inertia /*[nbody][3]*/, *body_invweight0 /*[nbody][2]*/;
    /* joints [njnt] */
    const int32_t *jnt_type, *jnt_bodyid, *jnt_qposadr, *jnt_dofadr, *jnt_limited;
    const double *jnt_pos, *jnt_axis /*[njnt][3]*/, *jnt_range /*[njnt][2]*/, *jnt_stiffness, *jnt_margin;
    const double *qpos0, *qpos_spring; /*[nq]*/
    /* dofs [nv] */
    const int32_t *dof_bodyid, *dof_jntid, *dof_parentid, *dof_madr /*[nv+1]*/;
    const double *dof_armature, *dof_damping, *dof_frictionloss, *dof_invweight0;
    /* geoms [ngeom] */
    const int32_t *geom_type, *geom_bodyid, *geom_contype, *geom_conaffinity, *geom_condim;
    const int32_t *geom_vertadr, *geom_vertnum;
    const double *geom_pos, *geom_quat, *geom_size /*[ngeom][3]*/, *geom_friction /*[ngeom][3]*/;
    const double *geom_margin, *geom_gap, *geom_solref /*[ngeom][2]*/, *geom_solimp /*[ngeom][5]*/;
    const double *geom_rbound, *geom_center /*[ngeom][3] body frame*/;
    const double *mesh_vert;       /* [nmeshvert][3], body frame */
    const int32_t *mesh_adjadr;    /* [nmeshvert+1] CSR */
    const int32_t *mesh_adj;       /* [nmeshadj] global vertex ids */
    const int32_t *exclude_pair;   /* [nexclude][2] body ids */
    /* actuators [nu]: motors on joints ([MJ-ext] joint transmission).  actuator_dofid = first dof of the joint; actuator_gear [nu][3]:
     * gear[0] scales the control on a hinge / slide dof, on a ball joint the generalised force on its three dofs is gear[0..2] * ctrl
     * (a torque vector in the child body's frame: uhc/khrylib/mocap/skeleton_mesh_v2.py:183-193 writes one such motor per bone axis) */
    const int32_t *actuator_dofid;
    const double *actuator_gear;
} UhcModelDesc;

/*
 * Controller constants of HumanoidEnv.do_simulation / compute_torque / rfc_implicit
 * (uhc/envs/humanoid_im.py:1014-1076, 1136-1190).
 */
typedef struct UhcCtrlDesc {
    int32_t n_substeps;   /* frame_skip, 15 (humanoid_im.py:64) */
    int32_t action_type;  /* 0 = "position" (stable PD), 1 = "torque" (humanoid_im.py:1157-1160) */
    int32_t meta_pd;      /* 0 none, 1 per-substep gains (30 numbers), 2 per-joint (humanoid_im.py:1054-1067) */
    int32_t rfc_mode;     /* 0 none, 1 implicit root wrench (humanoid_im.py:1136-1143), 2 explicit per-body wrenches (:1080-1132) */
    int32_t action_dim;   /* nu + vf_dim + meta_pd_dim (humanoid_im.py:250) */
    int32_t body_vf_dim;  /* explicit: 6 + 3 * residual_force_torque (humanoid_im.py:242) */
    double rfc_scale;     /* residual_force_scale * rfc_rate */
    double rfc_lim;       /* residual_force_lim */
    double base_rot[4];   /* data_specs.base_rot (humanoid_im.py:85) */
    const double *jkp, *jkd, *torque_lim, *a_scale; /* [nu] host arrays */
    const int32_t* vf_body; /* explicit: model body id of each residual-force body, in action order (humanoid_im.py:236-241) */
    int32_t n_vf_body;
    int32_t _pad;
} UhcCtrlDesc;

typedef struct UhcModel UhcModel;
typedef struct UhcBatch UhcBatch;

/* per-env state fields addressable through uhc_batch_field() */
enum UhcField {
    UHC_F_QPOS = 0,      /* [n_env][nq]   data.qpos */
    UHC_F_QVEL = 1,      /* [n_env][nv]   data.qvel */
    UHC_F_XPOS = 2,      /* [n_env][nbody][3] data.body_xpos (as left by the last forward pass) */
    UHC_F_XQUAT = 3,     /* [n_env][nbody][4] data.body_xquat */
    UHC_F_XIPOS = 4,     /* [n_env][nbody][3] data.xipos */
    UHC_F_QM = 5,        /* [n_env][nM]   data.qM (tree-sparse) */
    UHC_F_QFRC_BIAS = 6, /* [n_env][nv]   data.qfrc_bias */
    UHC_F_QACC = 7,      /* [n_env][nv]   data.qacc of the last forward pass (the warm start is kept separately) */
    UHC_F_CTRL = 8,      /* [n_env][nu]   data.ctrl of the last substep */
    UHC_F_NCON = 9,      /* int32 [n_env] data.ncon of the last forward pass */
    UHC_F_NEFC = 10,     /* int32 [n_env] data.nefc */
    UHC_F_FAIL = 11,     /* int32 [n_env] sticky physics-failure flag (NaN / huge qacc, qpos, qvel).  An env that fails at uhc_batch_set_state
                          * (a pose that is not a pose) keeps the qpos / qvel it was handed and runs NO forward pass: its derived fields
                          * (xpos, xquat, xipos, qM, qfrc_bias, qacc, ncon, nefc) are those of its PREVIOUS state and must not be read
                          * until the env has been given a valid state (the reference raises fail from do_simulation only,
                          * uhc/envs/humanoid_im.py:1207-1211; mj_forward on garbage returns garbage there) */
    UHC_F_SOLVER_ITER = 12, /* int32 [n_env] PGS sweeps used by the last solve */
    UHC_F_QFRC_APPLIED = 13, /* [n_env][nv] data.qfrc_applied of the last substep */
    UHC_F_EFC_OVERFLOW = 14, /* int32 [n_env] sticky: constraint rows were dropped (nefc cap) */
    UHC_F_STAGE_PROF = 15,   /* int64 [n_env][UHC_PROF_WORDS] per-stage shader-cycle counters (profiling builds), or the tier trace (UhcTraceWord) */
    UHC_F_REDO = 16,         /* int32 [n_env] bit 0: the env's last step / forward pass exceeded the fast tier's capacity (64 rows, 16 contacts, packed
                              * row storage, 12 body-body rows) and was computed by the general tier (128 rows, 64 contacts, 20 body-body rows), the
                              * large one (256 / 128 / 32; bit 6) or tier 4 (up to 1024 rows / 192-320 contacts / 128 body-body rows, by what the LDS holds beside the Hessian; bits 6 and 30), all of
                              * which solve the problem exactly: working sets of <= 64 rows on the dual QP in the general / large tier; Newton's method
                              * on the primal problem -- the reference's MuJoCo default -- in tier 4, which takes whatever the large tier cannot hold
                              * or whose working sets it cannot finish (an island with more than 64 force-carrying rows).  Bit 30: (part of) the step
                              * was solved by tier 4; bit 29: one of its Newton iterations stopped at the cap of 100 (the best iterate is used).
                              * Batches whose last tier is the large one (UHC_TIERS=3, or a model whose tier-4 layout does not fit 160 KiB of LDS)
                              * keep rounds 3-4's behaviour: such an island in windows of 64 rows to a KKT residual of 1e-9 (1 + max |b|) (bit 3: it
                              * happened, it is not a fallback); bit 1: in at least one substep the solve fell back to solver 0 (sweeps to tolerance;
                              * with tier 4 only for friction-loss rows); bits 2, 4, 5, diagnostic: why (friction-loss rows / no convergence of the
                              * working sets / a working set the pivoting could not solve); bit 8 + k: substep k (< 21) of the step was one of those
                              * (a checker that follows the same path needs to know which); bit 7: constraint rows / contacts beyond the LAST tier's
                              * capacity were DROPPED in this step (UHC_F_EFC_OVERFLOW is the sticky version, cleared by the env's next set_state);
                              * without tier 4 a forward pass that dropped rows gets a bounded exact attempt and at most 32 sweeps (bits 1 and 7).
                              * An env with friction-loss rows (dof_frictionloss > 0: box constraints) is solved by sweeps from the warm start at either solver, in
                              * every tier: the fast tier does so without a word (the word stays 0); at solver 1 the general tier, the large tier and tier 4 report
                              * bits 1 and 2 and the swept bit of every substep they computed, tier 4 without bit 30; at solver 0 the general and the large tier report
                              * bit 1 and the substep bits without a reason -- as for any env at solver 0 -- and tier 4 reports neither */
    UHC_F_TIER = 17,         /* int32 [n_env] 1 | 2 | 3 | 4: the tier the env's next step starts in under uhc_batch_set_kernel_path(2) */
    UHC_F_HANDON_WHY = 18,   /* int32 [n_env] diagnostic of the last step: bits 0-7 why the fast tier handed the env on, bits 8-15 why the general tier did
                              * (1 contacts, 2 constraint rows, 4 body-body row slots, 8 packed row storage, 16 MPR candidate list beyond the tier's
                              * capacity, 32 the working sets did not finish: more force-carrying rows in an island than a working set holds), bits 16-23 the
                              * substep of the last hand-on, bits 24-31 why the LARGE tier handed the env on to tier 4 (the same reason bits);
                              * 0 = the env stayed in the tier it started in */
    UHC_F_QACC_WARMSTART = 19, /* [n_env][nv] data.qacc_warmstart: what the next step's first solve starts from */
    UHC_F_COST = 20          /* int32 [n_env] how close the env's last step came to any capacity of the fast tier, in sixty-fourths: orders the fast tier's launch */
};
/* the bits of UHC_F_REDO (the prose above says what each means) */
#define UHC_REDO_GENERAL (1 << 0)       /* computed by the general tier, the large one or tier 4 */
#define UHC_REDO_SWEPT (1 << 1)         /* in at least one substep the solve fell back to sweeps */
#define UHC_REDO_WHY_FRICTION (1 << 2)  /* ... why: friction-loss rows */
#define UHC_REDO_WINDOWED (1 << 3)      /* an island was solved in windows of 64 rows (not a fallback) */
#define UHC_REDO_WHY_NOCONV (1 << 4)    /* ... why: no convergence of the working sets */
#define UHC_REDO_WHY_PIVOT (1 << 5)     /* ... why: a working set the pivoting could not solve */
#define UHC_REDO_LARGE (1 << 6)         /* computed by the large tier or tier 4 */
#define UHC_REDO_DROPPED (1 << 7)       /* rows / contacts beyond the last tier's capacity were dropped in this step */
#define UHC_REDO_SWEPT_SUBSTEP0 (1 << 8) /* UHC_REDO_SWEPT_SUBSTEP0 << k: substep k was solved by sweeps, k < UHC_REDO_SWEPT_SUBSTEPS */
#define UHC_REDO_SWEPT_SUBSTEPS 21
#define UHC_REDO_PRIMAL_CAP (1 << 29)   /* a Newton iteration of tier 4 stopped at its cap */
#define UHC_REDO_PRIMAL (1 << 30)       /* (part of) the step was solved by tier 4 */
/* UHC_F_HANDON_WHY: four fields of UHC_HANDON_FIELD's width; the reason bits of the three tiers' fields */
#define UHC_HANDON_FIELD 0xff
#define UHC_HANDON_FAST_SHIFT 0         /* why the fast tier handed the env on */
#define UHC_HANDON_GENERAL_SHIFT 8      /* why the general tier did */
#define UHC_HANDON_SUBSTEP_SHIFT 16     /* the substep of the last hand-on */
#define UHC_HANDON_LARGE_SHIFT 24       /* why the large tier handed the env on to tier 4 */
#define UHC_HANDON_CONTACTS 1
#define UHC_HANDON_ROWS 2
#define UHC_HANDON_DENSE_SLOTS 4
#define UHC_HANDON_ROW_STORAGE 8
#define UHC_HANDON_CANDIDATES 16
#define UHC_HANDON_SOLVER 32

/* UHC_DEBUG in the environment of uhc_batch_create: debug switches, OR-ed (KernelArgs::dbg) */
enum UhcDebug {
    UHC_DEBUG_NO_MERGE = 1 << 0,        /* the working sets never merge islands */
    UHC_DEBUG_NO_VSTAGE = 1 << 1,       /* MPR's vertices are not staged in LDS */
    UHC_DEBUG_RESTART_HANDON = 1 << 2,  /* a handed-on env restarts its step instead of resuming at the substep (only the whole-step launch can: no chunks) */
    UHC_DEBUG_ENV_ORDER = 1 << 3,       /* the sticky fast tier launches in env order */
    UHC_DEBUG_TRACE = 1 << 4,           /* tier trace in the stage-profile record (UhcTraceWord; tools/tier_trace.py) */
    UHC_DEBUG_NO_GATE = 1 << 5,         /* no gate before the fast tier's launch */
    UHC_DEBUG_LOG = 1 << 6,             /* log the queue lengths and the gate's wait per step, and tier 4's layout, to stderr */
    UHC_DEBUG_NO_BOX_CULL = 1 << 7,     /* no box cull of the convex pairs */
    /* Measurement switches: they change which envs report windows / sweeps in UHC_F_REDO, and exist only in libraries built with -DUHC_EXPERIMENTS (tools/ A/B
     * builds).  The shipped library compiles their reads out (UHC_EXP, uhc_physics_impl.h) and masks the bits (uhc_plan.cpp); uhc_build_flags() bit 0 tells which kind a library is. */
    UHC_DEBUG_EXP_NO_RANK_FILL = 1 << 8,   /* the general tier's first working set is NOT filled by rank (k_as_general; A/B of DESIGN 2) */
    UHC_DEBUG_EXP_FILL_48 = 1 << 9,        /* ... fill 48 lanes instead of 64 */
    UHC_DEBUG_EXP_FILL_56 = 1 << 10,       /* ... fill 56 */
    UHC_DEBUG_EXP_FIXED_CAP2 = 1 << 11,    /* a fixed cap UHC_Q2_MAX on the general tier's consumers (plan_sticky_step, uhc_plan.cpp) */
    UHC_DEBUG_EXP_STICKY_TIER4 = 1 << 12   /* sticky tier 4: an env whose step ended in tier 4 starts its next step there, at the head of the tier-4 consumers' queue
                                            * (next_tier, uhc_step_words.h; measured and not the default) */
};
#define UHC_DEBUG_EXP_MASK (UHC_DEBUG_EXP_NO_RANK_FILL | UHC_DEBUG_EXP_FILL_48 | UHC_DEBUG_EXP_FILL_56 | UHC_DEBUG_EXP_FIXED_CAP2 | UHC_DEBUG_EXP_STICKY_TIER4)

/* UHC_F_STAGE_PROF: UHC_PROF_WORDS int64 words per env, in two uses that overlay each other.  A library built with -DUHC_STAGE_PROF accumulates shader cycles per
 * stage in words 0 .. 39 (the stages' names: tools/stage_profile.py NAMES).  The shipped library writes the TIER TRACE there under UHC_DEBUG_TRACE: 100 MHz wall-clock
 * stamps and substeps of one control step, in the words below (the reader clears the record per step). */
#define UHC_PROF_WORDS 40
enum UhcTraceWord {
    UHC_TRACE_TAKEN = 0,           /* + 2 (tier - 1), tiers 1-3: when the tier took the env up */
    UHC_TRACE_LET_GO = 1,          /* + 2 (tier - 1), tiers 1-3: when it let the env go (done, or handed on) */
    UHC_TRACE_HANDON_SUBSTEP = 6,  /* + (tier - 1), tiers 1, 2: the substep at which the tier handed the env on */
    UHC_TRACE_CONSUMER = 8,        /* + UHC_TRACE_CONSUMER_WORDS (tier - 2), tiers 2, 3, in the record of env blockIdx: a queue consumer's own entry, first env claimed, exit, envs processed */
    UHC_TRACE_GATE = 16,           /* in the record of the LAST env, 5 words: the gate's start, its end, consumers reported in at its start / end, of how many */
    UHC_TRACE_TAKEN4 = 21,         /* tier 4's own stamps */
    UHC_TRACE_LET_GO4 = 22,
    UHC_TRACE_HANDON_SUBSTEP3 = 23,  /* the substep at which the large tier handed the env on to tier 4 */
    UHC_TRACE_CHUNK_WAIT = 24      /* the fast tier in chunks: ticks the env's later chunks spent waiting for the previous one (summed) */
};
#define UHC_TRACE_CONSUMER_WORDS 4

const char* uhc_last_error(void);
int32_t uhc_abi_version(void);
/* Which kind of build the library is: bit 0 = the solver's measurement switches (UHC_DEBUG_EXP_*) are compiled in (-DUHC_EXPERIMENTS, tools/ builds only),
 * bit 1 = per-stage cycle counters (-DUHC_STAGE_PROF), bit 2 = poisoned LDS, bit 3 = LDS guard words.  0 for the shipped library: a stray UHC_DEBUG cannot
 * change which solver path an env takes (tests/test_capi_symbols.py). */
int32_t uhc_build_flags(void);

/* model lifetime (host side) */
int32_t uhc_model_create(const UhcModelDesc* desc, UhcModel** out);
void uhc_model_free(UhcModel* m);
int32_t uhc_model_nM(const UhcModel* m);

/*
 * Create a batch of n_env environments on `device_id`.
 *   models[n_models]: distinct models; env_model[n_env] (host, may be NULL => all envs use
 *   models[0]) selects each env's model.  All models must share topology (sizes, tree, types);
 *   bodies may differ in geometry/inertia (the reference rebuilds the model per episode from
 *   SMPL shape: uhc/envs/humanoid_im.py:154-180).
 */
int32_t uhc_batch_create(const UhcModel* const* models, int32_t n_models, const int32_t* h_env_model,
                         int32_t n_env, int32_t device_id, const UhcCtrlDesc* ctrl, UhcBatch** out);
void uhc_batch_free(UhcBatch* b);
/* bind to an existing hipStream_t (e.g. torch's current stream); NULL = the device's null stream.
 * A new batch starts on a private non-blocking stream. */
int32_t uhc_batch_set_stream(UhcBatch* b, void* hip_stream);
int32_t uhc_batch_sync(UhcBatch* b);
/* change rfc_scale between iterations (rfc_decay: uhc/agents/agent_copycat.py:283-290) */
int32_t uhc_batch_set_rfc_scale(UhcBatch* b, double rfc_scale);

/* Which kernel tier computes a step.  The fused step kernel exists in four tiers: fast (<= 64 constraint rows / 16 contacts / 12
 * body-body rows per env; Delassus matrix in registers), general (<= 128 / 64 / 20; working sets; two workgroups per CU), large
 * (<= 256 / 128 / 32; a whole CU's LDS) and tier 4 (<= 1024 / 192-320 / 128, rows in HBM, the Hessian of MuJoCo's primal problem in LDS,
 * Newton's method -- the reference's default solver, whose cost does not depend on the number of rows).  A tier that cannot hold an env
 * leaves it untouched and hands it to the next one, from the substep that did not fit; in the chained launches tier 4 has no launch of its own (the large
 * tier's workgroup goes on with it); under sticky tiers (mode 2) it has queue consumers like the general and the large tier.  What exceeds the LAST tier is dropped and flagged (UHC_F_EFC_OVERFLOW; the reference's models ask
 * MuJoCo for njmax 2500 / nconmax 500, uhc/khrylib/mocap/skeleton_mesh.py:46).  UHC_TIERS=2 | 3 in the environment of uhc_batch_create
 * ends the chain at the general / large tier (rounds 2-4's behaviour, kept for A/B measurements).
 *   0 (default) = chain: the fast tier on every env, then the general tier on the envs it handed on, then the large tier;
 *   1 = the general tier first (then the large one): for scenes where nearly every env exceeds the fast tier;
 *   2 = sticky tiers: every env starts a step in the tier that computed its previous step (it comes down a tier only with room to
 *       spare), and the general / large tiers' own envs run on a side stream BESIDE the fast tier's -- their launches last several times
 *       longer per env, in a chain behind the fast tier the whole step would wait for them.  Results do not depend on the mode beyond
 *       rounding (every tier solves the same QP exactly), and a rerun of the same calls takes the same tiers.  Not capture-safe across
 *       uhc_batch_set_stream changes: the side stream forks from and joins the batch's stream with events.
 * UHC_F_REDO of a step: bit 0 = computed by the general or large tier (or tier 4), bit 1 = its exact solve swept in some substep (bits
 * 2-5 why, bits 8+ which substeps), bit 6 = computed by the large tier or tier 4, bit 30 = tier 4 (Newton on the primal).  Timing (uhc_batch_set_timing) brackets the fast tier's launch (modes
 * 0, 2) or the general tier's (mode 1). */
int32_t uhc_batch_set_kernel_path(UhcBatch* b, int32_t mode);

/* switch the contact solver of the dual QP between launches: solver 0 / 1 and the sweep cap, as in UhcModelDesc (MuJoCo's opt.solver /
 * opt.iterations are run-time options too); iterations <= 0 keeps the current cap */
int32_t uhc_batch_set_solver(UhcBatch* b, int32_t solver, int32_t iterations);

/* device pointer + element count of a state field (valid until uhc_batch_free) */
int32_t uhc_batch_field(UhcBatch* b, int32_t field, void** d_ptr, int64_t* count);

/*
 * MujocoEnv.set_state + sim.forward() (uhc/khrylib/rl/envs/common/mujoco_env.py:106-113) for the
 * envs listed in d_env_ids[n] (device int32; NULL => all n_env envs in order, n must be n_env).
 * d_qpos [n][nq], d_qvel [n][nv] are indexed by position in the list.  Clears the fail flag and
 * the warm start (sim.reset(): mujoco_env.py:96) of those envs.
 */
int32_t uhc_batch_set_state(UhcBatch* b, const int32_t* d_env_ids, int32_t n, const double* d_qpos,
                            const double* d_qvel);

/*
 * HumanoidEnv.do_simulation(action, frame_skip) (uhc/envs/humanoid_im.py:1145-1190) for every env:
 * n_substeps x { compute_torque -> clip -> ctrl; rfc_implicit -> qfrc_applied; sim.step() }.
 *   d_action      [n_env][action_dim]  policy output (joint residuals | residual force | meta-PD)
 *   d_target_base [n_env][nu]          expert joint pose of the next frame (get_expert_kin_pose(delta_t=1))
 *   d_active      int32 [n_env] or NULL: envs with 0 are left untouched (finished episodes)
 */
int32_t uhc_batch_simulate(UhcBatch* b, const double* d_action, const double* d_target_base,
                           const int32_t* d_active);

/* Measurement hook: while enabled, every uhc_batch_simulate brackets its fused step kernel (the fast variant
 * of uhc_step_kernel) with HIP events on the batch's stream; uhc_batch_kernel_time drains them (synchronising
 * on the events) and returns the summed kernel time and the number of launches since the last call. */
int32_t uhc_batch_set_timing(UhcBatch* b, int32_t enable);
int32_t uhc_batch_kernel_time(UhcBatch* b, double* total_ms, int32_t* launches);
/* Workgroups that gave up waiting since the batch was created (synchronises the batch's stream): queue consumers of the sticky tiers whose producers did
 * not run beside them, and workgroups of the chunked fast tier (UHC_FAST_CHUNK) whose env's previous chunk did not finish within 50 ms.  Nothing is
 * dropped when one does -- the chained launches / the workgroup that holds the env take over -- but a healthy run reports 0.
 * n_slow (may be NULL): queue consumers that left after 50 ms behind producers that WERE running beside them (some had finished) but had not all finished:
 * a sign of a very slow env-step in the tier below, not of launches that cannot overlap; the host does not act on it. */
int32_t uhc_batch_give_ups(UhcBatch* b, int32_t* n, int32_t* n_slow);

/* What the fast kernel does with an env that has more than 16 contacts or 64 constraint rows:
 * 0 (default) = leave it to the general kernel (exact, costs a second pass whenever one env overflows);
 * 1 = keep the first 16 contacts / the rows of the contacts that fit completely and carry on (MuJoCo itself drops
 *     contacts beyond nconmax); such envs are reported in UHC_F_EFC_OVERFLOW.  Rows that do not fit the packed
 *     row storage still go to the general kernel. */
int32_t uhc_batch_set_overflow_mode(UhcBatch* b, int32_t truncate);
/* mj_forward only (no control, no integration) on all envs: refreshes xpos/xquat/xipos/qM/qfrc_bias */
int32_t uhc_batch_forward(UhcBatch* b);

/* ------------------------------------------------------------------------------------------------
 * Env layer: what HumanoidEnv.step / reset / load_expert do around the physics, on device.
 * ---------------------------------------------------------------------------------------------- */
typedef struct UhcEnv UhcEnv;

/* constants of HumanoidEnv (uhc/envs/humanoid_im.py) and of the reward (uhc/losses/reward_function.py:12-36) */
typedef struct UhcEnvDesc {
    int32_t obs_v;               /* 2: get_full_obs_v2 (humanoid_im.py:419-503); 1: get_full_obs_v1 (:323-417); 6: get_full_obs_v6 (:596-666);
                                  * 3: get_full_obs_v3 (:758-767) = fut_frames v2 blocks, look-ahead 0, skip, 2 skip, ...;
                                  * 5: get_full_obs_v5 (:505-594); 0: get_full_obs (:290-317), shaped by obs_flags;
                                  * 4: get_full_obs_v4 (:769-861): its obs_full = global block (28) | shape (17) | one row of 26 per non-root body (hinge models) */
    int32_t has_shape;           /* append beta(16) + gender to the observation (humanoid_im.py:1390-1406) */
    int32_t env_episode_len;     /* cfg.env_episode_len */
    int32_t env_expert_trail_steps;
    int32_t ee_body[5];          /* model body ids of SMPL_EE_NAMES (smpl_parser.py:228) */
    int32_t reward_v;            /* 0: world_rfc_implicit_reward (reward_function.py:12-88) = world_rfc_implicit_reward_quat (:92-171);
                                  * 1: world_rfc_explicit_reward (:253-341); 2: world_rfc_implicit_v1_mul (:174-250);
                                  * 3: world_rfc_explicit_mul_reward (:346-430); 4: world_rfc_implicit_v2 (:643-723); 5: world_rfc_implicit_v3 (:726-820) */
    double body_diff_thresh;     /* humanoid_im.py:88-89 */
    double reward_weights[16];   /* w_p w_v w_e w_c w_vf k_p k_v k_e k_c k_vf | w_wp w_j k_wp k_j (reward_v 4, 5) | 0 0 */
    const double* jpos_diffw;    /* [nbody-1] SMPLConverter.get_new_diff_weight() (host) */
    int32_t fut_frames;          /* obs_v 3: cfg.fut_frames (default 10) */
    int32_t fut_skip;            /* obs_v 3: cfg.skip (default 10) */
    int32_t obs_flags;           /* obs_v 0: bit 0 cfg.obs_heading, bit 1 cfg.root_deheading, bit 2 cfg.obs_phase, bit 3 cfg.obs_vel == "root" */
    const double* reward_jpos_diffw; /* reward_v 4, 5: reward_weights["jpos_diffw"] [nbody-1] (host); NULL = ones */
    int32_t term_body;           /* cfg.env_term_body (humanoid_im.py:1223-1230): 0 "body" (mean body distance > body_diff_thresh), 1 "root" (root height
                                  * below the window's lowest expert root height - 0.1); "Head" reads a key the reference never sets */
    int32_t num_obj;             /* expert["num_obj"] (humanoid_im.py:1284-1287): free objects, the LAST num_obj bodies of the model (one free joint
                                  * each).  Observation, reward and termination read the humanoid in front of them -- qpos[:qpos_lim], qvel[:qvel_lim],
                                  * body_xpos[1:body_lim] (humanoid_im.py:113-115, 421-422) --, a reset puts the objects at obj_pose[ind] with zero velocity */
} UhcEnvDesc;

/* expert frame record layout of the clip bank (doubles; see uhc_amd/csrc/uhc_device_env.h) */
#define UHC_FRAME_STRIDE 584

enum UhcEnvField {
    UHC_E_OBS = 0,          /* [n_env][obs_dim] */
    UHC_E_REWARD = 1,       /* [n_env] */
    UHC_E_REWARD_PARTS = 2, /* [n_env][6] pose, vel, ee, com, vf, 0 (reward_v 4, 5: pose, world pose, body com, joint pos, vel, vf) */
    UHC_E_DONE = 3,         /* int32 [n_env] */
    UHC_E_FAIL = 4,         /* int32 [n_env] info["fail"] */
    UHC_E_END = 5,          /* int32 [n_env] info["end"] */
    UHC_E_PERCENT = 6,      /* [n_env] info["percent"] */
    UHC_E_CUR_T = 7,        /* int32 [n_env] */
    UHC_E_BODY_DIFF = 8,    /* [n_env] calc_body_diff() of the last step */
    UHC_E_TARGET_BASE = 9,  /* [n_env][nu] expert joint pose handed to the PD controller */
    UHC_E_CONSUMED = 10,    /* int32 [n_env] 1 where the last uhc_env_auto_reset() started the queued window, 0 elsewhere */
    UHC_E_EPISODE = 11,     /* [2][n_env] running episode length and return (reward + end * end_reward), kept by step / auto_reset */
    UHC_E_SNAPSHOT = 12,    /* [5][n_env] written by uhc_env_auto_reset: done, episode length, episode return, percent, consumed */
    UHC_E_MODEL = 13        /* int32 [n_env] which of the batch's models each env runs on now (assign / auto_reset / a live restart switch it); a batch created
                             * with ONE model keeps no such array: the field is refused there */
};

int32_t uhc_env_create(UhcBatch* b, const UhcEnvDesc* desc, UhcEnv** out);
void uhc_env_free(UhcEnv* e);
int32_t uhc_env_obs_dim(const UhcEnv* e);
int32_t uhc_env_field(UhcEnv* e, int32_t field, void** d_ptr, int64_t* count);
/* clip bank (device pointers, borrowed: must outlive the env or the next set_bank):
 * d_frames [n_frames][UHC_FRAME_STRIDE], d_clip_start int32 [n_clips], d_clip_beta [n_clips][17] */
int32_t uhc_env_set_bank(UhcEnv* e, const double* d_frames, int64_t n_frames, const int32_t* d_clip_start,
                         const double* d_clip_beta, int32_t n_clips);
/* expert["obj_pose"] of every frame of the bank (device pointer, borrowed): d_obj_pose [n_frames][7 num_obj], object k at columns
 * 7k .. 7k + 6 (position, quaternion wxyz); reset / auto_reset read the row of the window's first frame (reset_model, humanoid_im.py:
 * 1284-1287: init_pose = concat(expert pose, obj_pose[0]), init_vel = concat(expert velocity, zeros)).  Call after uhc_env_set_bank. */
int32_t uhc_env_set_obj_pose(UhcEnv* e, const double* d_obj_pose, int64_t n_frames);
/* Per-clip body shape (the reference rebuilds the MuJoCo model from the clip's beta in load_expert -> reset_robot,
 * humanoid_im.py:154-180,204): d_clip_model int32 [n_clips] (borrowed, NULL to switch off) names, for every clip of the
 * bank, which of the batch's models (uhc_batch_create) its episodes run on; assign / auto_reset switch the env's model. */
int32_t uhc_env_set_clip_models(UhcEnv* e, const int32_t* d_clip_model);
/* load_expert (humanoid_im.py:182-215): env d_env_ids[i] tracks frames [fr_start, fr_start+fr_len) of clip d_clip_ids[i] */
int32_t uhc_env_assign(UhcEnv* e, const int32_t* d_env_ids, int32_t n, const int32_t* d_clip_ids,
                       const int32_t* d_fr_start, const int32_t* d_fr_len);
/* Episode turnover without a host round trip (the reference's sampler does `load_expert; reset` on the worker, agent_copycat.py:
 * 526-531, right after `done`): uhc_env_set_next queues, per env, the window its NEXT episode will track (+ the reset noise,
 * d_noise [n][nu] or NULL); uhc_env_auto_reset then does, for every env whose done flag is set, load_expert + reset_model on
 * the device (queued window if there is one, else the current window again) and refreshes its observation row.  The done
 * flags are left as the step wrote them; UHC_E_CONSUMED tells which envs took their queued window.  Of the reset's sim.forward()
 * only the kinematics run here (UHC_F_XPOS / XQUAT / XIPOS, the observation); its dynamics half (qM, qfrc_bias, qacc of the reset
 * state) runs at the head of the env's next uhc_env_step, so UHC_F_QM / QFRC_BIAS / QACC / NCON / NEFC of a restarted env are those
 * of its previous episode until then.  The steps that follow are bit-identical to those after uhc_env_assign + uhc_env_reset. */
int32_t uhc_env_set_next(UhcEnv* e, const int32_t* d_env_ids, int32_t n, const int32_t* d_clip_ids, const int32_t* d_fr_start,
                         const int32_t* d_fr_len, const double* d_noise);
int32_t uhc_env_auto_reset(UhcEnv* e);
/* bonus added to the reward of a step that ends its clip (Agent: `if end_reward and info["end"]: reward += env.end_reward`,
 * uhc/khrylib/rl/agents/agent.py:84-85); UHC_E_REWARD stays the plain imitation reward, the episode return includes the bonus */
int32_t uhc_env_set_end_reward(UhcEnv* e, double end_reward);
/* MujocoEnv.reset -> reset_model (humanoid_im.py:1245-1299): state <- expert frame 0 (+ d_noise [n][nu] on the
 * joint angles, may be NULL), forward pass, observation written to the obs rows of those envs */
int32_t uhc_env_reset(UhcEnv* e, const int32_t* d_env_ids, int32_t n, const double* d_noise);
/* HumanoidEnv.step for every env with d_active != 0 (NULL = all): PD target gather, do_simulation,
 * cur_t += 1, termination, reward, next observation */
int32_t uhc_env_step(UhcEnv* e, const double* d_action, const int32_t* d_active);

/* ------------------------------------------------------------------ live targets: each env imitates a stream of frames appended while it runs
 * The per-env, per-step form of uhc_expert_frames (below): a kinematic policy, a pose estimator or a teleoperation source emits the next target pose every
 * control step (the reference's uhc/envs/humanoid_kin_v1.py puts a frozen copycat policy under such a source), and uhc_env_live_push turns that qpos row into
 * the frame record the env kernels read -- no host FK, no upload, no uhc_env_set_bank.  (Purely additive: UHC_ABI_VERSION stays 11.)
 *
 * uhc_env_live_begin  allocates a live bank [n_env][cap][UHC_FRAME_STRIDE] OWNED BY THE ENV and installs it as the env's clip bank: clip i is env i's
 *                     stream, clip_start[i] = i cap.  Memory: n_env x cap x 4 672 B for the bank (1 024 envs x cap 512: 2.45 GB) + n_env x (76 + 17) x 8 B
 *                     + 2 n_models x 576 B.  n_body, h_parent, h_ee_body, d_body_pos, d_body_ipos [n_models][24][3], dt: as in uhc_expert_frames; the two
 *                     device tables are COPIED (nothing stays borrowed).  d_beta [n_env][17] or NULL (zeros): what has_shape observations append.
 *                     n_models must be the batch's model count; the per-env model selector is the batch's own (uhc_env_set_clip_models is switched off).
 *                     Refused: cap < 2, n_body != 24, a parent table or end effector uhc_expert_frames refuses, dt not > 0, another n_models, an env
 *                     created with num_obj > 0.  A second call with cap <= the allocated one reuses the memory and clears every stream.
 *                     Every slot starts as zeros and every env's window as frame 0 of its own stream: a reset or step before the first push reads zeros.
 * uhc_env_live_push   ONE launch on the batch's stream; no allocation, no host synchronisation, no host read: it can be captured into a graph.
 *                     d_env_ids int32 [n], d_qpos [n][76] (rows as uhc_expert_frames'), d_root_quat_record [n][4] or NULL (written into the record's
 *                     qpos[3:7] instead of d_qpos' quaternion, which kinematics and velocities keep reading), d_restart int32 [n] or NULL, d_model int32
 *                     [n] or NULL.  Row r, env = d_env_ids[r]:
 *                       env outside [0, n_env): the row is ignored; no read or write goes through the index.
 *                       d_restart[r] != 0: the row becomes frame 0 of a NEW stream, with the one-frame-clip record (zero qvel, bangvel); the stream's length
 *                         is 1, its lowest root height the row's, dropped = 0; d_model[r] (outside 0 .. n_models - 1: 0) becomes the env's model.
 *                       otherwise the row is appended at L = the stream's length (after the slide, where uhc_env_live_slide is on): L == 0 (no stream) or
 *                         L == cap: dropped[env] += 1, nothing else is written.  Else slot L gets the record of the pair (previous row, row); when the row is
 *                         the stream's frame 1 (L == 1 and nothing has slid off), frame 0's qvel and bangvel are overwritten
 *                         with this record's (cat(qvel[0:1], qvel)): the stream's records ARE uhc_expert_frames' of the same rows, bit for bit.
 *                       Offsets come from the env's current model.  cur_t, done, the observation and the simulation state are not touched: after pushing the
 *                       head of a stream the caller resets with uhc_env_reset(ids).
 *                     Each env may appear at most ONCE per call (the caller's duty): a duplicate may lose a row, it cannot reach outside the arrays.
 *                     n == 0 succeeds and launches nothing.
 * uhc_env_live_view   device pointers: d_frames [n_env][cap][UHC_FRAME_STRIDE], d_len int32 [n_env], d_dropped int32 [n_env]; any may be NULL.
 * uhc_env_live_end    leaves the env WITHOUT a bank (the live memory stays the env's, for the next live_begin, until uhc_env_free); uhc_env_set_bank
 *                     while live ends live mode the same way and installs the caller's bank.
 * In live mode uhc_env_assign, uhc_env_set_next, uhc_env_auto_reset, uhc_env_set_clip_models and uhc_env_set_obj_pose return an error that says so: a
 * stream has no window to assign or queue; a done env is restarted with push(restart) + uhc_env_reset.
 *
 * What the env kernels make of a stream (they clamp every expert read to the stream's length - 1; step number t reads frame t + 1 for the PD target and
 * the reward, frame t + 2 (+ k skip) for the next observation):
 *   - with frames 0 .. t + 2 pushed before uhc_env_step number t, target, reward, termination and observation are exactly those of a clip;
 *   - with fewer, the newest frame stands in for the missing ones;
 *   - `end` is raised when cur_t >= len - 1 + env_expert_trail_steps -- the stream has run dry -- or at env_episode_len;
 *   - `percent` is cur_t / (len - 1) with the length at that moment;
 *   - observation v3 looks fut_frames skip frames ahead and sees the newest frame for whatever is not there yet.
 *
 * Endless streams: the window slides (off by default; uhc_env_live_begin switches it off and clears base and moved).
 * uhc_env_live_slide  on != 0: from now on uhc_env_live_push makes room before it appends, for every listed env whose stream is FULL (len == cap): the S =
 *                     min(start_ind + cur_t, len - 1) records behind the frame the env reads next are discarded, the others move to the front of the env's
 *                     slice (one more launch in front of the append, on the batch's stream; no allocation, no host read: still capturable), and len, the
 *                     env's window length and its internal start index drop by S.  What a slide keeps: every frame the env kernels can still read -- the
 *                     current one (observation v0), cur_t + 1 and the look-aheads -- and always the newest, so a stream that has run dry keeps holding it.
 *                     Target, reward, termination, `end`, cur_t and the observations are those of a stream that never slid, bit for bit; a bank of cap =
 *                     a few times the producer's lead serves a session of any length.  S == 0 on a full stream (the env has not stepped since the last
 *                     slide): the row is dropped and counted as without sliding.  An env that is not listed, a foreign id and a restart row are not slid.
 *                     on == 0: pushes stop sliding; the window stays readable where it is, the next push to a full stream is dropped.
 *                     Refused: not in live mode; obs_v 0 with the phase word (obs_flags & 4), whose cur_t / len would jump at a slide.
 *                     Under sliding, `percent` is cur_t / (len - 1) of the WINDOW at that moment and is no progress measure; height_lb stays the minimum
 *                     over the whole stream since the restart; uhc_env_reset WITHOUT a restart row re-seats the env on the window's oldest kept frame
 *                     (slot 0), not on the stream's first frame, which is gone.  After a restart row, push the head and uhc_env_reset BEFORE the stream
 *                     fills: until the reset the env's cur_t is the old episode's, and a slide would discard the head's frames behind it.
 * uhc_env_live_window device pointers d_base, d_moved int32 [n_env]; either may be NULL.  base[env]: frames slid off since the restart -- the global index of
 *                     the frame in slot i of uhc_env_live_view is base[env] + i, and base + len is the number of frames the stream has accepted.
 *                     moved[env]: records copied by slides since the restart (what sliding costs).  Both are 0 while sliding was never switched on. */
int32_t uhc_env_live_begin(UhcEnv* e, int32_t cap, int32_t n_body, const int32_t* h_parent, const int32_t* h_ee_body, const double* d_body_pos,
                           const double* d_body_ipos, int32_t n_models, double dt, const double* d_beta);
int32_t uhc_env_live_push(UhcEnv* e, const int32_t* d_env_ids, int32_t n, const double* d_qpos, const double* d_root_quat_record,
                          const int32_t* d_restart, const int32_t* d_model);
int32_t uhc_env_live_view(UhcEnv* e, double** d_frames, int32_t** d_len, int32_t** d_dropped, int32_t* cap);
int32_t uhc_env_live_end(UhcEnv* e);
int32_t uhc_env_live_slide(UhcEnv* e, int32_t on);
int32_t uhc_env_live_window(UhcEnv* e, int32_t** d_base, int32_t** d_moved);

/* ------------------------------------------------------------------ rollout bookkeeping (one control step of the sampling loop)
 * The reference's sample_worker (uhc/khrylib/rl/agents/agent.py:60-100) does, per env step on the host: running_state(state),
 * select_action, memory.push, reward / mask bookkeeping.  Batched on the device these are launch-latency bound (~80 framework launches
 * per step); the entries below do them in a handful.  Free functions: all pointers are device pointers, `stream` is a hipStream_t
 * (NULL = the default stream), every reduction has a fixed order (bit-reproducible).  Layouts: states [n_env][T][obs_dim], actions
 * [n_env][T][act_dim], rewards / dones [n_env][T], mean_flags [T][n_env] (1.0 = take the mean action), d_t = the pass's step counter. */

/* memory.push(state, action, ...) + PolicyGaussian.select_action's sampling (policy_gaussian.py:22-31, distributions.py:6-25):
 * states[:, t] = state; action = mean where mean_flags[t] != 0 else mean + exp(log_std) * noise; actions[:, t] = action = d_action */
int32_t uhc_rollout_act(void* stream, int32_t n_env, int32_t T, const int64_t* d_t, int32_t obs_dim, int32_t act_dim, const double* d_state,
                        const double* d_mean, const double* d_log_std, const double* d_noise, const double* d_mean_flags, double* d_states,
                        double* d_actions, double* d_action);
/* agent.py:80-92: rewards[:, t] = reward + end * end_reward, dones[:, t] = done, c_reward_sum += sum(reward),
 * c_info_sum[k] += sum(parts[:, k]) (LoggerRL.step, logger_rl.py:29-33); n_parts <= 8.  d_redo (may be NULL): UHC_F_REDO of the step;
 * d_redo_counts (int64 [7]): [0] += envs the general / large tier or tier 4 computed, [1] += envs whose exact contact solve fell back to
 * sweeps, [2] += envs that lost constraint rows beyond the last tier's capacity in this step, [3] += envs the large tier or tier 4 computed,
 * [4] += envs with an island of more than 64 force-carrying rows solved exactly in windows of 64 rows (three-tier batches), [5] += envs
 * solved by Newton on the primal in tier 4, [6] += envs in which that iteration stopped at its cap (diagnostics) */
int32_t uhc_rollout_record(void* stream, int32_t n_env, int32_t T, const int64_t* d_t, const double* d_reward, const int32_t* d_done,
                           const int32_t* d_end, const double* d_end_reward, const double* d_parts, int32_t parts_stride, int32_t n_parts,
                           double* d_rewards, double* d_dones, double* d_c_reward_sum, double* d_c_info_sum, const int32_t* d_redo,
                           int64_t* d_redo_counts);
/* RunningStat.push for a batch (zfilter.py:17-27; Chan et al. merge, mathematically the rows pushed one by one): (n, mean, S) <-
 * merged with the rows of d_x [n_rows][dim] whose d_weights entry is non-zero (NULL = all rows).  d_scratch: uhc_filter_scratch_doubles */
int64_t uhc_filter_scratch_doubles(int32_t n_rows, int32_t dim);
int32_t uhc_filter_push(void* stream, const double* d_x, int32_t n_rows, int32_t dim, const int32_t* d_weights, double* d_n, double* d_mean,
                        double* d_S, double* d_scratch);
/* ZFilter.__call__ (zfilter.py:55-64): out = clip((x - mean) / (std + 1e-8), +-clip); std = sqrt(S / (n - 1)) (n <= 1: |mean|);
 * clip == 0: no clipping.  d_t_inc (may be NULL): incremented by one -- the step counter, this being the last launch of a step */
int32_t uhc_filter_apply(void* stream, const double* d_x, int32_t n_rows, int32_t dim, const double* d_n, const double* d_mean, const double* d_S,
                         int32_t demean, int32_t destd, double clip, double* d_out, int64_t* d_t_inc);

/* ------------------------------------------------------------------ expert frame records of a clip bank, computed on the device
 * Replaces Humanoid.qpos_fk (uhc/smpllib/torch_smpl_humanoid.py:234-261: Euler angles -> joint quaternions, forward kinematics, the two finite
 * differences) and the feature half of HumanoidEnv.load_expert (uhc/envs/humanoid_im.py:182-215) for a whole bank in ONE launch: a free function
 * like uhc_rollout_*, `stream` a hipStream_t (NULL = the default stream).
 *   n_body           24: UHC_FRAME_STRIDE is a 24-body layout
 *   h_parent [24]    HOST: parent of every body behind the world body, -1 for the root (body 0); a parent precedes its child
 *   h_ee_body [5]    HOST: indices 0 .. 23 of SMPL_EE_NAMES among those bodies
 *   d_body_pos, d_body_ipos [n_models][24][3]: model.body_pos / body_ipos behind the world body
 *   d_qpos [n_frames][76]: root position, root quaternion wxyz, 23 x 3 Euler angles (z, y, x) in the model's body order; the clips one after another
 *   d_clip_start int32 [n_clips], ascending from 0; the last clip ends at n_frames (as in uhc_env_set_bank)
 *   d_clip_model int32 [n_clips] or NULL (= model 0 for every clip): whose offsets a clip's frames are computed with
 *   d_root_quat_record [n_frames][4] or NULL: written into the record's qpos[3:7] INSTEAD of d_qpos' quaternion; kinematics and velocities keep
 *                    reading d_qpos (the ball-joint humanoid's second conversion: uhc/envs/humanoid_im.py:193-200)
 *   dt               frame time of the clips (1 / 30)
 *   d_frames [n_frames][UHC_FRAME_STRIDE]: out.  Slots 505 .. 511 are written as zeros.
 * Frame t >= 1 of a clip differences frames (t - 1, t); frame 0 takes frame 1's velocities; no difference reaches across a clip boundary.
 * A clip of ONE frame gets zero qvel and bangvel (the reference cannot compute such a clip at all).  qvel is clipped to +-10, bangvel is not.
 * Every argument is checked before the first HIP call; n_frames == 0 succeeds and launches nothing. */
int32_t uhc_expert_frames(void* stream, int32_t n_body, const int32_t* h_parent, const int32_t* h_ee_body, const double* d_body_pos,
                          const double* d_body_ipos, int32_t n_models, const double* d_qpos, int64_t n_frames, const int32_t* d_clip_start,
                          const int32_t* d_clip_model, int32_t n_clips, const double* d_root_quat_record, double dt, double* d_frames);

/* ------------------------------------------------------------------ AMASS poses -> qpos rows on the device
 * The step in front of uhc_expert_frames: smpl_to_qpose (uhc/smpllib/smpl_mujoco.py:543-607) as ONE launch over (frame, joint).  Per joint: rotation vector
 * -> quaternion (scipy's from_rotvec, no canonical sign) -> intrinsic ZYX Euler angles by scipy's quaternion algorithm, gimbal-lock branches included (X = 0
 * at lock); the root of the 76-wide row keeps a quaternion, formed through the rotation matrix with the reference converter's branch rule.  Free function
 * like uhc_expert_frames: `stream` is a hipStream_t (NULL = the default stream); every argument is checked before the first HIP call; n_frames == 0 succeeds
 * and launches nothing; no atomics (two runs are bit-identical); whatever the clip tables hold, no read or write leaves the arrays -- a d_clip_start that does
 * not ascend can only name the wrong clip, a d_clip_model outside 0 .. n_models - 1 reads as 0.  (Purely additive: UHC_ABI_VERSION stays 11.)
 *   n_joint 24; h_smpl_to_model [24] (HOST): the SMPL joint model slot m takes -- a permutation of 0 .. 23 with entry 0 = 0;
 *   d_root_offset [n_models][3]: each body shape's body_pos[1], added to the root position (NULL: count_offset=False);
 *   d_pose_aa [n_frames][72]; d_trans [n_frames][3] (NULL: (0, 0, 0.91437225) for every frame);
 *   d_clip_start int32 [n_clips], d_clip_model int32 [n_clips] (NULL: model 0 for every clip): which body shape's offset a frame gets;
 *   d_qpos [n_frames][76]: position, root quaternion (w, x, y, z), 23 x (Z, Y, X); d_qpos_quat [n_frames][99]: position, 24 x (w, x, y, z).  Either may be
 *   NULL, not both; both are 16-byte aligned. */
int32_t uhc_smpl_qpos(void* stream, int32_t n_joint, const int32_t* h_smpl_to_model, const double* d_root_offset, int32_t n_models,
                      const double* d_pose_aa, const double* d_trans, int64_t n_frames, const int32_t* d_clip_start, const int32_t* d_clip_model,
                      int32_t n_clips, double* d_qpos, double* d_qpos_quat);
/* uhc_smpl_qpos from 6D rows (smpl_6d_to_qpose, uhc/smpllib/smpl_mujoco.py:776-780): d_full_6d [n_frames][147] = translation | 24 x (column 0, column 1 of the
 * joint's rotation matrix: process_amass_db.convert_aa_to_orth6d's layout), 8-byte aligned.  Per joint x = a / |a|, z = (x x b) / |x x b|, y = z x x, the
 * quaternion of that matrix with w >= 0; behind it the same code as uhc_smpl_qpos.  A degenerate pair (a = 0, b parallel to a) gives NaN, as on the host. */
int32_t uhc_smpl6d_qpos(void* stream, int32_t n_joint, const int32_t* h_smpl_to_model, const double* d_root_offset, int32_t n_models, const double* d_full_6d,
                        int64_t n_frames, const int32_t* d_clip_start, const int32_t* d_clip_model, int32_t n_clips, double* d_qpos, double* d_qpos_quat);

/* ------------------------------------------------------------------ qpos rows -> SMPL poses on the device
 * The way back: qpos_to_smpl (uhc/smpllib/smpl_mujoco.py:738-752) and the first half of convert_2_smpl_params (uhc/envs/humanoid_im.py:127-133) as ONE launch
 * over (row, joint).  Per joint: the hinge triple (Z, Y, X) -> quaternion (scipy's from_euler, intrinsic) or, for the root and for ball joints, the
 * (w, x, y, z) quaternion normalised (from_quat) -> rotation vector (as_rotvec: w < 0 negates, exactly w == 0 does not; the series at or below 1e-3) and / or the
 * first two columns of its rotation matrix.  Free function like uhc_smpl_qpos: `stream` is a hipStream_t (NULL = the default stream); every argument is checked
 * before the first HIP call; n_seq == 0 succeeds and launches nothing; no index or counter, whatever it holds, sends a read or a write outside the arrays.
 * (Purely additive: UHC_ABI_VERSION stays 11.)
 *   n_joint 24; h_smpl_to_model [24] (HOST): as for uhc_smpl_qpos; ball: 0 = hinge rows (>= 76 wide: position, root (w, x, y, z), 23 x (Z, Y, X) in model order),
 *   1 = ball-joint rows (>= 99 wide: position, 24 x (w, x, y, z));
 *   d_qpos, row_stride: global row g = s * row_cap + r -- row r of sequence s -- lies at d_qpos + g * row_stride (in doubles, >= the width; 8-byte aligned, read
 *   16 bytes a lane where stride and base allow it).  So one entry point reads the simulation's qpos field (row_cap 1, stride nq), an evaluation record's
 *   d_pred_qpos ([n_env][row_cap][nqh] with the record's d_rows) and the clip bank's UHC_FR_QPOS columns (stride UHC_FRAME_STRIDE);
 *   d_seq_rows int32 [n_seq] or NULL (= every row): only rows r < d_seq_rows[s], clamped to 0 .. row_cap, are converted; every other output slot keeps what it held;
 *   d_seq_model int32 [n_seq] or NULL (= model 0): whose d_root_offset [n_models][3] a sequence's rows lose; an entry outside 0 .. n_models - 1 reads as 0;
 *   d_root_offset NULL: no offset (count_offset=False);
 *   d_pose_aa [n_seq * row_cap][72] in SMPL joint order; d_trans [..][3] = qpos[:3] - root_offset; d_full_6d [..][147] = trans | 24 x (column 0, column 1).
 *   Each may be NULL, not all three; each is 16-byte aligned.
 *   d_bad int32 [1]: set by the call to the number of converted rows with a quaternion of zero or non-finite norm, or a hinge triple that is not finite (scipy
 *   raises on a zero quaternion): such a row is NaN in every output.  h_bad (HOST, may be NULL): when given, the call waits for the stream and stores the count. */
int32_t uhc_qpos_smpl(void* stream, int32_t n_joint, const int32_t* h_smpl_to_model, int32_t ball, const double* d_root_offset, int32_t n_models,
                      const double* d_qpos, int64_t row_stride, int32_t n_seq, int32_t row_cap, const int32_t* d_seq_rows, const int32_t* d_seq_model,
                      double* d_pose_aa, double* d_trans, double* d_full_6d, int32_t* d_bad, int32_t* h_bad);

/* ------------------------------------------------------------------ evaluation on the device: trajectory record and imitation metrics
 * Replaces the host half of eval_seq (uhc/agents/agent_copycat.py:438-494: per control step, copies of qpos / xpos / the expert frame / done / reward /
 * percent and Python lists per clip) and compute_metrics (uhc/smpllib/smpl_eval.py:66-126).  Free functions like uhc_rollout_* and uhc_expert_frames:
 * `stream` is a hipStream_t (NULL = the default stream); every argument is checked before the first HIP call; n_env == 0 succeeds and launches nothing;
 * reductions have a fixed order and no floating-point atomics (two runs are bit-identical); no counter or index, whatever it holds, sends a read or a
 * write outside the arrays.  (Purely additive: UHC_ABI_VERSION stays 11.)
 *
 * The record belongs to the CALLER (zeroed before an episode batch):
 *   d_rows, d_steps int32 [n_env]      rows / rewards written so far
 *   d_pred_qpos [n_env][row_cap][nqh]  the humanoid's part of qpos
 *   d_pred_jpos [n_env][row_cap][72]   bodies 1 .. 24 of xpos
 *   d_gt_frame int64 [n_env][row_cap]  bank frame of the row: d_clip0[e] + min(t, d_len[e] - 1)
 *   d_rewards [n_env][row_cap]
 *   d_fail_safe int32 [n_env], d_percent [n_env], d_tele int32 [n_env], d_overflow int32 [1]
 * uhc_eval_record takes one snapshot for the envs with d_alive[e] != 0 (the mask handed to uhc_env_step):
 *   phase 0 (before the step): appends a row.
 *   phase 1 (after it): d_rewards[e][d_steps[e]++] = d_reward[e]; where d_done[e], appends a row with the same t, then -- fail_safe != 0 and
 *           d_percent_in[e] != 1 -- sets d_fail_safe[e] = d_tele[e] = 1 (the caller teleports the env to the expert pose and the episode goes on), or else
 *           clears d_alive[e] and writes d_percent[e].  d_tele is rewritten for EVERY env by every phase-1 call (0 where nothing is to teleport).
 * A row that does not fit row_cap is counted in d_overflow and not written.
 *   n_body 24; nq, nbody: row widths of d_qpos [n_env][nq] and d_xpos [n_env][nbody][3] (body 0 = the world; objects behind the humanoid);
 *   nqh: 7 .. nq.  d_done, d_reward, d_percent_in may be NULL in phase 0. */
int32_t uhc_eval_record(void* stream, int32_t phase, int32_t n_env, int32_t n_body, int32_t nq, int32_t nqh, int32_t nbody, int32_t row_cap, int32_t t,
                        int32_t fail_safe, const double* d_qpos, const double* d_xpos, const int64_t* d_clip0, const int32_t* d_len,
                        const int32_t* d_done, const double* d_reward, const double* d_percent_in, int32_t* d_alive, int32_t* d_rows,
                        int32_t* d_steps, double* d_pred_qpos, double* d_pred_jpos, int64_t* d_gt_frame, double* d_rewards, int32_t* d_fail_safe,
                        double* d_percent, int32_t* d_tele, int32_t* d_overflow);
/* compute_metrics for every env of a record against the bank d_frames [n_frames][UHC_FRAME_STRIDE] (gt root pose at UHC_FR_QPOS, gt joints at UHC_FR_WBPOS).
 *   d_row_metrics [n_env][row_cap][6]: root_dist (divided by the env's row count), vel_dist, accel_dist, mpjpe_g, pa_mpjpe, mpjpe, in mm.  An env with T rows
 *                  gets T rows, T - 1 for vel_dist, T - 2 for accel_dist (numpy's lengths); every other slot is left untouched.
 *   d_clip_means [n_env][6]: the means over those rows; over no row: NaN (np.mean of an empty array).
 *   d_bad int32 [1]: set by the call to the number of read d_gt_frame entries outside [0, n_frames).  Such an entry is not followed: every output that
 *                  would read it (the row's six, and the velocity / acceleration of the one or two rows before it) is NaN.
 *   h_bad (HOST, may be NULL): when given, the call waits for the stream and stores d_bad's count there; otherwise it is asynchronous like the rest. */
int32_t uhc_eval_metrics(void* stream, int32_t n_env, int32_t n_body, int32_t nqh, int32_t row_cap, const int32_t* d_rows, const double* d_pred_qpos,
                         const double* d_pred_jpos, const int64_t* d_gt_frame, const double* d_frames, int64_t n_frames, double* d_row_metrics,
                         double* d_clip_means, int32_t* d_bad, int32_t* h_bad);

/* ------------------------------------------------------------------ contact quality of a motion: penetration, skate, float, contact count
 * compute_penetration / compute_skate (uhc/smpllib/smpl_eval.py:125-149) on the device.  The reference scores SMPL surface vertices; this library scores the
 * convex-hull vertices every compiled model carries in the body frame (mesh hulls; sphere and capsule cores with their radius) -- a DEVIATION; the SMPL
 * vertices themselves are uhc_smpl_mesh's, below, from the caller's own model files -- and adds
 * `float`, which the reference does not have.  Same conventions as the evaluation functions above: `stream` is a hipStream_t (NULL = the default stream),
 * every argument is checked before the first HIP call, reductions have a fixed order and no floating-point atomics (two runs are bit-identical), no index or
 * counter, whatever it holds, sends a read or a write outside the arrays.  (Purely additive: UHC_ABI_VERSION stays 11.)
 *
 * World vertex w = xpos[b] + R(xquat[b]) v for a vertex v of body b; height h = w.z - radius - floor_z; float64, products and sums rounded separately.
 * Per row r of a sequence of T rows, in mm:
 *   pen[r]      -mean(h over the vertices with h < 0) * 1000; 0 when there is none
 *   skate[r]    r <= T - 2: mean of |w_xy[r + 1] - w_xy[r]| * 1000 over the vertices with h <= 0 in both rows; 0 when there is none
 *   float[r]    min(h) * 1000 when every vertex has h > 0, else 0
 *   contact[r]  the number of vertices with h <= 0, as a double
 * A row whose n_body poses hold a non-finite number gets NaN in its four values and in the skate of the row before it, and counts 1 in d_bad.
 *
 * uhc_surface_create copies the host tables to the device (the current one): h_vert_body int32 [n_vert] (0 .. n_body - 1), h_vert_radius [n_vert] or NULL
 *   (all zero), h_vert [n_models][n_vert][3]: the same topology on n_models body shapes.  Refused: n_body outside 1 .. 64, n_vert outside 1 .. 65535,
 *   n_models < 1, a body outside the range, a negative or non-finite radius, a non-finite vertex.
 * uhc_surface_metrics scores n_seq sequences.  Row i of sequence s is global row d_seq_start[s] + i (i < d_seq_rows[s], clamped to 0 .. row_cap); its
 *   positions lie at d_pos + global_row * pos_stride as [n_body][3], its quaternions (w, x, y, z) at d_quat + global_row * quat_stride as [n_body][4]; the
 *   strides are in doubles.  So one entry point reads a pose record (uhc_eval_record_pose: stride 168, offsets 0 and 72) and the clip bank (stride
 *   UHC_FRAME_STRIDE, base pointers at the frames' world body positions and quaternions, offsets 151 and 223).
 *   d_seq_model int32 [n_seq] or NULL: the body shape of each sequence; an entry outside 0 .. n_models - 1 reads as 0.
 *   d_row_out [n_rows_total][4]: pen, skate, float, contact of every global row of a sequence (skate: not of its last row); other slots are left untouched.
 *   d_seq_means [n_seq][4]: the means over T, T - 1, T, T rows in row order; over no row: NaN.
 *   d_bad int32 [1]: set by the call to the number of rows with a non-finite pose plus the number of sequences whose rows would leave 0 .. n_rows_total
 *                  (such a sequence is skipped: nothing of it is read or written).
 *   h_bad (HOST, may be NULL): when given, the call waits for the stream and stores d_bad's count there.  n_seq == 0 succeeds and launches nothing.
 * uhc_eval_record_pose appends xpos[1 .. 24] and xquat[1 .. 24] of every env uhc_eval_record's rule selects (d_alive[e] != 0, and phase == 0 or d_done[e], and
 *   0 <= d_rows[e] < row_cap) to row d_rows[e] of d_pose [n_env][row_cap][168] (72 position doubles, then 96 quaternion doubles).  It reads d_rows and does
 *   not write it: enqueue it on the same stream directly BEFORE uhc_eval_record of the same snapshot, which advances the counter.  d_done may be NULL in phase 0. */
typedef struct UhcSurface UhcSurface;
int32_t uhc_surface_create(int32_t n_body, int32_t n_vert, int32_t n_models, const int32_t* h_vert_body, const double* h_vert_radius, const double* h_vert,
                           UhcSurface** out);
void uhc_surface_free(UhcSurface* s);
int32_t uhc_surface_metrics(void* stream, const UhcSurface* surf, int32_t n_seq, const int64_t* d_seq_start, const int32_t* d_seq_rows, int32_t row_cap,
                            const int32_t* d_seq_model, const double* d_pos, int64_t pos_stride, const double* d_quat, int64_t quat_stride,
                            int64_t n_rows_total, double floor_z, double* d_row_out, double* d_seq_means, int32_t* d_bad, int32_t* h_bad);
int32_t uhc_eval_record_pose(void* stream, int32_t phase, int32_t n_env, int32_t nbody, int32_t row_cap, const double* d_xpos, const double* d_xquat,
                             const int32_t* d_done, const int32_t* d_alive, const int32_t* d_rows, double* d_pose);

/* ------------------------------------------------------------------ the SMPL body mesh: vertices, joints and contact quality on SMPL vertices
 * SMPL_Parser.get_joints_verts (uhc/smpllib/smpl_parser.py:335-360: smplx's lbs) and compute_penetration / compute_skate on its vertices
 * (uhc/smpllib/smpl_eval.py:113-149) as one fused kernel, float64.  The SMPL tables come from the caller's own (licensed) model files; nothing of them is
 * shipped.  Same conventions as the functions above: `stream` is a hipStream_t (NULL = the default stream), every argument is checked before the first HIP
 * call, reductions have a fixed order and no floating-point atomics (two runs are bit-identical), no index or counter, whatever it holds, sends a read or a
 * write outside the arrays.  (Purely additive: UHC_ABI_VERSION stays 11.)
 *
 *   R_j      = I + sin(a) K + (1 - cos(a)) K K,  a = |r_j + 1e-8| (1e-8 added to each component, as smplx), K = skew(r_j / a): exactly I at r_j = 0
 *   v_shaped = v_template + shapedirs beta;  J = J_regressor v_shaped                                   (per sequence)
 *   v_posed  = v_shaped + posedirs feature,  feature = (R_1 .. R_23 - I) row-major, 207 numbers         (on v_mfma_f64_16x16x4_f64)
 *   G_j      = chain over the parents of [R_j | J_j - J_parent(j)];  A_j = [G_j.R | G_j.t - G_j.R J_j]
 *   vertex   = (sum_j w[v][j] A_j) [v_posed; 1] + trans;  joint_j = G_j.t + trans
 * and, with h = vertex.z - floor_z and radius 0, the four values of uhc_surface_metrics (pen, skate, float, contact: same definitions, units, strict /
 * non-strict predicates and T / T - 1 / T / T means), plus the lowest vertex z of a row.
 *
 * uhc_smpl_mesh_create copies the tables of n_models bodies (the genders) that share n_vert and the 24-joint tree to the current device, in the layout the
 *   kernel reads: h_v_template [n_models][n_vert][3], h_shapedirs [..][n_vert][3][10], h_posedirs [..][n_vert][3][207], h_J_regressor [..][24][n_vert],
 *   h_weights [..][n_vert][24], h_parents int32 [24] (parent[0] = -1).  Refused: n_vert outside 1 .. 65535, n_models < 1, a parent table that is
 *   no tree rooted at joint 0 with parent[j] < j, a non-finite table entry.  A handle serves one stream at a time: it owns what a call keeps between its
 *   kernels, and a call that needs more of it than any call before frees and allocates inside the call (hipFree / hipMalloc: not under stream capture; a
 *   first call of the largest shape outside the capture settles it).
 * uhc_smpl_mesh: rows are addressed as in uhc_surface_metrics (d_seq_start, d_seq_rows clamped to 0 .. row_cap, d_seq_model, n_rows_total); the pose of a
 *   global row lies at d_pose_aa + row * pose_stride as [72], its translation at d_trans + row * trans_stride as [3] (strides in doubles: uhc_qpos_smpl's
 *   outputs are read where they lie); d_betas [n_seq][10].
 *   Outputs, each may be NULL (not all): d_vert [n_rows_total][n_vert][3], d_joints [n_rows_total][24][3], d_row_out [n_rows_total][4], d_seq_means
 *   [n_seq][4], d_row_zmin [n_rows_total].  Slots of rows outside every sequence are left untouched.
 *   d_bad int32 [1]: set by the call to the number of rows with a non-finite pose or translation (NaN in every output of the row and in the skate of the
 *   row before it) plus the number of sequences whose rows would leave 0 .. n_rows_total (skipped: nothing of them is read or written).
 *   h_bad (HOST, may be NULL): when given, the call waits for the stream and stores d_bad's count there.  n_seq == 0 succeeds and launches nothing. */
typedef struct UhcSmplMesh UhcSmplMesh;
int32_t uhc_smpl_mesh_create(int32_t n_vert, int32_t n_models, const double* h_v_template, const double* h_shapedirs, const double* h_posedirs,
                             const double* h_J_regressor, const double* h_weights, const int32_t* h_parents, UhcSmplMesh** out);
void uhc_smpl_mesh_free(UhcSmplMesh* mesh);
int32_t uhc_smpl_mesh(void* stream, UhcSmplMesh* mesh, int32_t n_seq, const int64_t* d_seq_start, const int32_t* d_seq_rows, int32_t row_cap,
                      const int32_t* d_seq_model, const double* d_betas, const double* d_pose_aa, int64_t pose_stride, const double* d_trans,
                      int64_t trans_stride, int64_t n_rows_total, double floor_z, double* d_vert, double* d_joints, double* d_row_out,
                      double* d_seq_means, double* d_row_zmin, int32_t* d_bad, int32_t* h_bad);

/* ------------------------------------------------------------------ a frozen policy: raw observations -> action means, without the framework
 * The mean action of PolicyGaussian (uhc/khrylib/rl/core/policy_gaussian.py:9-31) and PolicyMCP (uhc/models/policy_mcp.py:9-37) behind the observation
 * filter ZFilter(update = False) (uhc/khrylib/utils/zfilter.py:55-64), float64, products on v_mfma_f64_16x16x4_f64.  Same conventions as the functions above:
 * `stream` is a hipStream_t (NULL = the default stream), every argument is checked before the first HIP call, every sum has a fixed order and no atomics (two
 * runs are bit-identical; a row's action is bit-identical whatever the batch size and wherever the row sits in the batch), no value in any array can send a
 * read or a write outside the arrays.  (Purely additive: UHC_ABI_VERSION stays 11.)
 *
 * A policy is a list of nets, each a chain of layers y = act(x W^T + b) on the filtered observation.  UHC_POLICY_GAUSSIAN: one net, the trunk and its linear
 * head (last width act_dim).  UHC_POLICY_MCP: n_nets - 1 primitive nets of equal shape (last width act_dim), then the composer (last width n_nets - 1, its
 * last layer activated like the others), mean = sum_p softmax(composer)_p mean_p.
 *
 * uhc_policy_create: h_n_layers int32 [n_nets]; h_widths / h_acts int32, the nets' layers one after the other (sum of h_n_layers entries): each layer's
 *   output width and its activation (UHC_ACT_*; UHC_ACT_GELU is the exact erf form); h_w / h_b: per layer, in the same order, HOST arrays in nn.Linear layout
 *   ([out][in], [out]).  The weights are copied to the current device and repacked there once.  Refused by name: a non-positive dimension, an unknown
 *   activation, primitives of unequal shape, a composer whose last width is not the number of primitives, a non-finite weight.  max_rows: the largest n_rows
 *   of a uhc_policy_act; the handle owns what a call keeps between its kernels (nothing is allocated in a call), so it serves one stream at a time.
 * uhc_policy_set_filter: the frozen statistics of the filter from the HOST: n, h_mean [obs_dim], h_S [obs_dim] (RunningStat's sum of squared deviations:
 *   std = sqrt(S / (n - 1)), |mean| while n <= 1), demean, destd, clip (0 = none): y = clip((x - mean) / (std + 1e-8), +-clip), the arithmetic of
 *   uhc_filter_apply -- the filtered observation has the same bits.  h_mean = h_S = NULL, or no call at all: observations go in as they are.  Waits for the device.
 * uhc_policy_set_params: new weights for the same shapes, per layer as in uhc_policy_create; on_device != 0: DEVICE arrays (the live parameters of a policy
 *   that is still being trained), else HOST arrays (checked for non-finite entries; device arrays are not read by the host).  Copied and repacked on `stream`.
 *   Host arrays are the caller's again when the call returns (it waits for `stream`); device arrays must stay valid and unchanged until the work enqueued on
 *   `stream` has run -- the call does not wait for it.
 * uhc_policy_act: d_obs: row r at d_obs + r * obs_stride (in doubles, >= obs_dim: a view into a wider array is read where it lies); d_state_out
 *   [n_rows][obs_dim] or NULL: the filtered observation; d_mean [n_rows][act_dim]; d_weight_out [n_rows][n_primitives] or NULL (MCP only): the composer's
 *   weights.  One launch per layer (all nets at once) plus one for the MCP sum, a straight chain on `stream`: it may be captured in a HIP graph.
 *   n_rows == 0 succeeds and launches nothing; n_rows > max_rows and obs_stride < obs_dim are refused.
 * uhc_policy_save / uhc_policy_load: a flat little-endian file: the 8 bytes "UHCPOLCY", int32 version (1), kind, obs_dim, act_dim, n_nets, n_layers [n_nets],
 *   widths, acts; int32 has_filter, demean, destd, 0; double clip, n, mean [obs_dim], S [obs_dim]; then per net and layer W [out][in] and b [out] as doubles.
 *   The round trip is bit-exact.  save waits for the device.  uhc_policy_dims: what a loaded handle holds (any pointer may be NULL); packed_bytes: the size of
 *   the repacked weights and biases a call reads. */
enum { UHC_POLICY_GAUSSIAN = 0, UHC_POLICY_MCP = 1 };
enum { UHC_ACT_NONE = 0, UHC_ACT_TANH = 1, UHC_ACT_RELU = 2, UHC_ACT_SIGMOID = 3, UHC_ACT_GELU = 4 };
typedef struct UhcPolicy UhcPolicy;
int32_t uhc_policy_create(int32_t kind, int32_t obs_dim, int32_t act_dim, int32_t max_rows, int32_t n_nets, const int32_t* h_n_layers,
                          const int32_t* h_widths, const int32_t* h_acts, const double* const* h_w, const double* const* h_b, UhcPolicy** out);
void uhc_policy_free(UhcPolicy* policy);
int32_t uhc_policy_dims(const UhcPolicy* policy, int32_t* kind, int32_t* obs_dim, int32_t* act_dim, int32_t* max_rows, int32_t* n_primitives,
                        int64_t* packed_bytes);
int32_t uhc_policy_set_filter(UhcPolicy* policy, double n, const double* h_mean, const double* h_S, int32_t demean, int32_t destd, double clip);
int32_t uhc_policy_set_params(void* stream, UhcPolicy* policy, const double* const* w, const double* const* b, int32_t on_device);
int32_t uhc_policy_act(void* stream, UhcPolicy* policy, int32_t n_rows, const double* d_obs, int64_t obs_stride, double* d_state_out, double* d_mean,
                       double* d_weight_out);
int32_t uhc_policy_save(const UhcPolicy* policy, const char* path);
int32_t uhc_policy_load(const char* path, int32_t max_rows, UhcPolicy** out);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* UHC_AMD_H */
