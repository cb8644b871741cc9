"""The cases of tests/test_gpu_passives.py (friction-loss rows, joint springs, slide joints on every tier), their oracle trajectories and their bars.

Nothing here touches a device.  tests/test_passives_cpu.py walks the same list and proves, on the oracle alone, that every case reaches what it is there for (its tier's
band of rows and contacts at every step, one friction row per dof with friction loss, a slide limit row where one is claimed, friction rows at both bounds and inside them):
the GPU file may then compare every env of every case, with nothing skipped or filtered.

THE BAR of a quantity is max(10 x the oracle's own sensitivity, the bar of the nearest existing test).  The sensitivity is the largest deviation, over the case's
trajectory, between the oracle run from the case's state and the oracle run from that state perturbed by 1e-14 in qpos and qvel (tools/chaos_probe.py's experiment): the
device differs from the oracle by summation order alone -- a few ulps per operation -- and 1e-14 is about a hundred ulps of these states already, hence the factor 10.
The floors: 1e-13 kinematics, 1e-11 qM, 1e-9 bias (test_forward_fields_match_oracle); qacc 1e-8 + 1e-9 |qacc| where both sides solve exactly (test_exact_solver_forward)
and 1e-5 + 1e-6 |qacc| where both sweep to tolerance (test_forward_fields_match_oracle); per-step qpos / qvel against the free-running oracle 1e-8
(test_oracle_decides_its_own_solver).  The derived part for qpos / qvel must stay below 1e-8 in every case (asserted on the CPU): a case that breaches it gets a shorter
trajectory, never a wider cap.  The bars come from the oracle alone, never from device output."""
import dataclasses
import functools

import numpy as np

from tests.helpers import caterpillar_model, passive_ctrl, slider_model, with_passives

PERTURBATION = 1e-14
FACTOR = 10.0
FLOOR = dict(xpos=1e-13, xquat=1e-13, xipos=1e-13, qM=1e-11, qfrc_bias=1e-9, qpos=1e-8, qvel=1e-8)
QACC_FLOOR_EXACT = (1e-8, 1e-9)  # (atol, rtol): both sides at the QP's exact optimum, or no rows at all
QACC_FLOOR_SWEPT = (1e-5, 1e-6)  # both sides sweep to the model's tolerance
CAP_QPOS_QVEL = 1e-8             # the derived bar of qpos / qvel stays below this in every case
FORWARD_FIELDS = ("xpos", "xquat", "xipos", "qM", "qfrc_bias", "qacc")

# the tiers' bands of (rows, contacts): what a step must show for the tier a case is named for to be the one that computes it
FAST_ROWS, FAST_CON, GENERAL_ROWS, GENERAL_CON, LARGE_ROWS = 64, 16, 128, 64, 256


def in_band(tier, nefc, ncon):
    if tier == "fast":
        return nefc <= FAST_ROWS and ncon <= FAST_CON
    if tier == "general":
        return (FAST_ROWS < nefc <= GENERAL_ROWS and ncon <= GENERAL_CON) or (FAST_CON < ncon <= GENERAL_CON and nefc <= GENERAL_ROWS)
    if tier == "large":
        return GENERAL_ROWS < nefc <= LARGE_ROWS
    if tier == "beyond_fast":  # the general tier in some substeps, the large one in others
        return FAST_ROWS < nefc <= LARGE_ROWS
    return nefc > LARGE_ROWS  # tier 4


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    tier: str              # the tier every env of the case belongs to at every step: fast | general | large | tier4 (| beyond_fast: general or large)
    models: tuple          # one model, or several of one topology (env_model picks)
    env_model: tuple       # per env
    ctrl: object
    qpos: np.ndarray       # [n_env][nq]
    qvel: np.ndarray       # [n_env][nv]
    act: np.ndarray        # [steps][n_env][action_dim]: raw motor torques (the humanoid: stable-PD actions)
    target: np.ndarray     # [n_env][max(nu, 1)]: the PD target's base (unused by torque control)
    slide_limit: bool = False  # the case claims a slide limit row (in some env at some step)

    @property
    def n_env(self):
        return len(self.env_model)

    @property
    def steps(self):
        return self.act.shape[0]

    def model_of(self, e):
        return self.models[self.env_model[e]]


# ------------------------------------------------------------------ the slider (slide - hinge - slide, no contacts)
def slider_states(n, seed):
    """Seeded states of slider_model(): slide positions on both sides of qpos0, every fourth env beyond the rail's limit (alternately below and above)."""
    rng = np.random.default_rng(seed)
    q = np.c_[rng.uniform(-0.25, 0.35, n), rng.normal(scale=0.6, size=n), rng.uniform(-0.2, 0.2, n)]
    q[0::8, 0], q[4::8, 0] = -0.3 - rng.uniform(0.001, 0.02, len(q[0::8])), 0.4 + rng.uniform(0.001, 0.02, len(q[4::8]))
    v = rng.normal(scale=0.5, size=(n, 3))
    return q, v


SLIDER_SPRING = dict(stiffness=np.array([40.0, 6.0, 25.0]), qpos_spring=np.array([0.12, -0.4, -0.07]))


def _slider_case(name, model, steps, seed, n_env=4, qv=None, slide_limit=False):
    q, v = slider_states(n_env, seed) if qv is None else qv
    act = np.random.default_rng(seed + 100).normal(scale=1.0, size=(steps, len(q), 3))
    return Case(name, "fast", (model,), (0,) * len(q), passive_ctrl(model, n_substeps=3), q, v, act, np.zeros((len(q), 3)), slide_limit)


def _edge_states():
    """One state and its mirror image (the rail's limits are not symmetric: neither is beyond them)."""
    q = np.array([[0.1, 0.5, -0.08]])
    v = np.array([[0.3, -0.4, 0.2]])
    return np.r_[q, -q], np.r_[v, -v]


# ------------------------------------------------------------------ the caterpillar on the floor
def caterpillar_state(m, seed, lift, scale, vel):
    rng = np.random.default_rng(seed)
    q = m.qpos0.copy()
    q[2] += lift
    q[7:] = rng.normal(scale=scale, size=m.nq - 7)
    return q, rng.normal(scale=vel, size=m.nv)


# (n_seg, tier, the seeds of its envs, lift, hinge noise, speed): chosen on the oracle so that every step stays inside the tier's band (tests/test_passives_cpu.py proves it)
CATERPILLARS = ((4, "fast", (4, 5), 0.0002, 0.02, 0.05), (6, "general", (0, 2), -0.0004, 1e-3, 0.01),
                (12, "large", (0, 2), -0.0004, 1e-3, 0.01), (27, "tier4", (1, 2), -0.0004, 1e-3, 0.01))
CATERPILLAR_FLOSS, CATERPILLAR_STIFFNESS = 0.5, 20.0
# the mixed batch: the 4-segment animal with and without friction loss, interleaved over 8 envs
MIXED_SEEDS = (4, 5, 8, 9, 10, 16, 22, 29)


def _caterpillar_case(n_seg, tier, seeds, lift, scale, vel, solver, steps=10):
    m = with_passives(dataclasses.replace(caterpillar_model(n_seg), solver=solver), frictionloss=CATERPILLAR_FLOSS, stiffness=CATERPILLAR_STIFFNESS)
    qv = [caterpillar_state(m, s, lift, scale, vel) for s in seeds]
    n = len(seeds)
    return Case(f"caterpillar{n_seg}_solver{solver}", tier, (m,), (0,) * n, passive_ctrl(m, n_substeps=1), np.stack([q for q, _ in qv]), np.stack([v for _, v in qv]),
                np.zeros((steps, n, 1)), np.zeros((n, 1)))


def _mixed_case(steps=10):
    base = dataclasses.replace(caterpillar_model(4), solver=1)
    models = (with_passives(base, frictionloss=0.0, stiffness=CATERPILLAR_STIFFNESS), with_passives(base, frictionloss=CATERPILLAR_FLOSS, stiffness=CATERPILLAR_STIFFNESS))
    n_seg, tier, _, lift, scale, vel = CATERPILLARS[0]
    qv = [caterpillar_state(base, s, lift, scale, vel) for s in MIXED_SEEDS]
    n = len(qv)
    return Case("mixed_batch", "fast", models, tuple(e % 2 for e in range(n)), passive_ctrl(base, n_substeps=1), np.stack([q for q, _ in qv]), np.stack([v for _, v in qv]),
                np.zeros((steps, n, 1)), np.zeros((n, 1)))


# ------------------------------------------------------------------ the humanoid the configs describe
HUMANOID_FLOSS, HUMANOID_STIFFNESS = 1.0, 5.0


def _humanoid_case(steps=10, n=2):
    import os
    from uhc_amd.sim import load_asset_model, make_ctrl
    base = load_asset_model()
    ctrl = make_ctrl(base)
    m = with_passives(dataclasses.replace(base, solver=1), frictionloss=HUMANOID_FLOSS, stiffness=HUMANOID_STIFFNESS)
    z = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uhc_amd", "assets", "standing_neutral.npz"))
    rng = np.random.default_rng(4)  # (the states and the action scale of test_contact_trajectory_200_steps)
    qpos = np.tile(z["qpos"], (n, 1))
    qpos[:, 7:] += rng.normal(scale=0.02, size=(n, m.nu))
    qvel = rng.normal(scale=0.05, size=(n, m.nv))
    act = np.random.default_rng(5).normal(scale=0.05, size=(steps, n, ctrl.action_dim))
    return Case("humanoid_passives", "beyond_fast", (m,), (0,) * n, ctrl, qpos, qvel, act, qpos[:, 7:].copy())


@functools.lru_cache(maxsize=None)
def cases():
    sl = slider_model()
    eq, ev = _edge_states()
    out = [
        _slider_case("slider_spring", with_passives(dataclasses.replace(sl, solver=1), **SLIDER_SPRING), 10, 31, qv=tuple(a[[1, 2, 3, 5]] for a in slider_states(8, 31))),
        _slider_case("slider_friction", with_passives(dataclasses.replace(sl, solver=1), frictionloss=np.array([0.5, 0.05, 0.3])), 10, 32, qv=tuple(a[[1, 2, 3, 5]] for a in slider_states(8, 32))),
        _slider_case("slider_spring_friction_limit", with_passives(dataclasses.replace(sl, solver=1), frictionloss=np.array([0.5, 0.05, 0.3]), **SLIDER_SPRING), 10, 33,
                     qv=tuple(a[[0, 4, 1, 2]] for a in slider_states(8, 33)), slide_limit=True),
    ]
    # two sweeps and no more: far from converged, the forces are what the ORDER of the rows makes them -- friction-loss rows first, then the limits (the rail's friction row
    # and its limit row share one Jacobian); a tolerance-terminated solve hides a swapped order below any bar
    out.append(_slider_case("slider_friction_limit_two_sweeps", with_passives(dataclasses.replace(sl, solver=1, iterations=2), frictionloss=np.array([0.5, 0.05, 0.3]), **SLIDER_SPRING), 10, 35,
                            qv=tuple(a[[0, 4, 8, 12]] for a in slider_states(16, 35)), slide_limit=True))
    for floss, tag in ((1e-9, "tiny"), (0.5, "half"), (1e9, "huge")):
        out.append(_slider_case(f"friction_bound_{tag}", with_passives(dataclasses.replace(sl, solver=1), frictionloss=floss), 10, 34, qv=(eq, ev)))
    for spec in CATERPILLARS:
        for solver in (0, 1):
            out.append(_caterpillar_case(*spec, solver))
    out.append(_mixed_case())
    out.append(_humanoid_case())
    return tuple(out)


def case(name):
    return {c.name: c for c in cases()}[name]


CASE_NAMES = ("slider_spring", "slider_friction", "slider_spring_friction_limit", "slider_friction_limit_two_sweeps", "friction_bound_tiny", "friction_bound_half", "friction_bound_huge") + \
    tuple(f"caterpillar{s[0]}_solver{k}" for s in CATERPILLARS for k in (0, 1)) + ("mixed_batch", "humanoid_passives")


# ------------------------------------------------------------------ the oracle's trajectories
def _run(c, e, dq=0.0):
    """Env e of case c on the free-running oracle (its own solver decisions), from the case's state + dq.  Per control step: qpos, qvel, nefc, ncon; at the state and
    after every step the rows' kinds, bounds and forces; the first forward pass's fields."""
    from oracle.physics import OracleSim
    m = c.model_of(e)
    o = OracleSim(m, c.ctrl)
    rng = np.random.default_rng(12345 + e)
    q = c.qpos[e] + dq * rng.choice([-1.0, 1.0], size=m.nq)
    v = c.qvel[e] + dq * rng.choice([-1.0, 1.0], size=m.nv)
    o.set_state(q, v)
    first = {k: o.get(k).copy() for k in FORWARD_FIELDS}
    rows = []

    def look():
        rows.append(dict(type=o.get("efc_type").astype(int), floss=o.get("efc_floss").copy(), force=o.get("efc_force").copy(), J=o.get("efc_J").reshape(-1, m.nv).copy(),
                         nefc=o.geti("nefc"), ncon=o.geti("ncon"), fail=o.geti("fail")))
    look()
    qs, vs = [], []
    for t in range(c.steps):
        o.do_simulation(c.act[t, e], c.target[e])
        look()
        qs.append(o.get("qpos").copy())
        vs.append(o.get("qvel").copy())
    return dict(first=first, rows=rows, qpos=np.stack(qs) if qs else np.zeros((0, m.nq)), qvel=np.stack(vs) if vs else np.zeros((0, m.nv)), nefc=np.array([r["nefc"] for r in rows]), ncon=np.array([r["ncon"] for r in rows]),
                max_nefc=o.geti("max_nefc"), max_ncon=o.geti("max_ncon"), fail=max(r["fail"] for r in rows))


def qacc_floor(c, run):
    """(atol, rtol) of the first forward pass's qacc: exact on both sides without rows, or at solver 1 without friction-loss rows; sweeps to tolerance otherwise."""
    r0 = run["rows"][0]
    exact = r0["nefc"] == 0 or (c.models[0].solver == 1 and not (r0["type"] == 1).any())
    return QACC_FLOOR_EXACT if exact else QACC_FLOOR_SWEPT


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's runs of every env of the case (shared by the CPU and the GPU file, computed once), the sensitivities and the bars."""
    c = case(name)
    runs = [_run(c, e) for e in range(c.n_env)]
    pert = [_run(c, e, PERTURBATION) for e in range(c.n_env)]
    sens = {k: max(float(np.abs(a[k] - b[k]).max()) for a, b in zip(runs, pert)) for k in ("qpos", "qvel")}
    for k in FORWARD_FIELDS:
        sens[k] = max(float(np.abs(a["first"][k] - b["first"][k]).max()) for a, b in zip(runs, pert))
    bars = {k: max(FACTOR * sens[k], FLOOR[k]) for k in FLOOR}
    qa = max(np.abs(r["first"]["qacc"]).max() for r in runs)
    at, rt = max((qacc_floor(c, r) for r in runs))
    bars["qacc"] = max(FACTOR * sens["qacc"], at + rt * qa)
    return dict(case=c, runs=runs, sens=sens, bars=bars)


def bar_table(names=CASE_NAMES):
    lines = [f"{'case':32s} " + " ".join(f"{k:>9s}" for k in ("qpos", "qvel", "qacc")) + "   (10 x sensitivity | bar)"]
    for n in names:
        r = reference(n)
        lines.append(f"{n:32s} " + " ".join(f"{FACTOR * r['sens'][k]:9.1e}" for k in ("qpos", "qvel", "qacc")) + " | " + " ".join(f"{r['bars'][k]:9.1e}" for k in ("qpos", "qvel", "qacc")))
    return "\n".join(lines)


# ------------------------------------------------------------------ the forward-field cases of the slider (16 seeded states, with and without springs)
@functools.lru_cache(maxsize=None)
def forward_case(springs):
    sl = dataclasses.replace(slider_model(), solver=1)
    m = with_passives(sl, **SLIDER_SPRING) if springs else sl
    q, v = slider_states(16, 41)
    return Case("slider_forward_springs" if springs else "slider_forward_plain", "fast", (m,), (0,) * 16, passive_ctrl(m, n_substeps=1), q, v, np.zeros((0, 16, 3)), np.zeros((16, 3)), True)


@functools.lru_cache(maxsize=None)
def forward_reference(springs):
    c = forward_case(springs)
    runs = [_run(c, e) for e in range(c.n_env)]
    pert = [_run(c, e, PERTURBATION) for e in range(c.n_env)]
    sens = {k: max(float(np.abs(a["first"][k] - b["first"][k]).max()) for a, b in zip(runs, pert)) for k in FORWARD_FIELDS}
    bars = {k: max(FACTOR * sens[k], FLOOR[k]) for k in FORWARD_FIELDS if k != "qacc"}
    qa = max(np.abs(r["first"]["qacc"]).max() for r in runs)
    at, rt = max(qacc_floor(c, r) for r in runs)
    bars["qacc"] = max(FACTOR * sens["qacc"], at + rt * qa)
    return dict(case=c, runs=runs, sens=sens, bars=bars)
