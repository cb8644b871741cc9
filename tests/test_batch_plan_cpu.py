"""The batch plan on the CPU: uhc_amd/csrc/uhc_plan.cpp (pure host C++, no HIP runtime) compiled with the host compiler beside a thin probe
(tests/plan_probe.cpp) and asked for the plan of every model class the GPU tests and bench.py run.

a. Invariants of the LDS layouts, the schedules, the marks, the guard table, the sticky-step sizes and the step's table of launches: what the kernels rely on and
   nothing else states.
b. Equality with tests/batch_plan_recording.json: the plan words and table hashes the unrefactored uhc_batch_create gave for the same inputs (recorded once, at the
   commit before the planner was split out, from that commit's uhc_capi.cpp compiled host-only with stand-ins for the hip* calls), and the outputs of the sticky
   launch arithmetic lifted from its launch()."""
import ctypes as C
import dataclasses
import itertools
import json
import os
import re

import numpy as np
import pytest

from tests import probe_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uhc_amd", "csrc")
RECORDING = os.path.join(ROOT, "tests", "batch_plan_recording.json")
KIB = 1024
N_ENVS = (1024, 4096)
CLASSES = ("asset", "generated", "ball", "ball_boxes", "rounded", "chain32")
KNOB_CASES = ("UHC_TIERS=2", "UHC_TIERS=3", "UHC_FAST_DENSE=40,6", "UHC_GUARD_LDS=1", "UHC_TIER_MARKS=60,20,10,50,16,8,8,6")
STICKY_GRID = dict(est2=(0, 5, 64, 300, 700, 900), est3=(0, 3, 40, 370), est4=(0, 2, 30), large_first=(0, 1), queues_off=(0, 1), n_env=N_ENVS)


def sticky_inputs():
    """[est2, est3, est4, est2_then, handed2, n_env, n_cu, lds_bytes_fast, large_first, last_tier, queues_off, q2_div, q2_wait_min, q2_max, q3_max, q4_max, dbg]: the grid
    above on 256 CUs, a 52 KiB fast layout, four tiers and the default caps; a third of the general tier's queue came in during the step."""
    g = STICKY_GRID
    return [[e2, e3, e4, e2, e2 // 3, n, 256, 52 * KIB, lf, 4, qo, 1, 16, 256, 32, 16, 0]
            for e2, e3, e4, lf, qo, n in itertools.product(g["est2"], g["est3"], g["est4"], g["large_first"], g["queues_off"], g["n_env"])]


def model_class(name):
    """-> (model, ctrl): the builders of the GPU tests and bench.py"""
    from tests.helpers import box_triangles, caterpillar_model, passive_ctrl
    from uhc_amd.model.mjcf import add_free_bodies
    from uhc_amd.sim import load_asset_model, make_ctrl
    from uhc_amd.smpllib.smpl_robot import robot_variant
    base = load_asset_model()
    if name == "asset":
        return base, make_ctrl(base)
    if name == "generated":  # configs[1]: body-body collisions on, rel_joint_lm ranges (bench.py GENERATED_CLASS)
        m = robot_variant(base, {"mesh": True, "model": "smpl"})
        return m, make_ctrl(m)
    if name in ("ball", "ball_boxes"):  # copycat_ball_1.yml's robot block; configs[4]: + four free 5 kg boxes of 0.3 m
        m = robot_variant(base, {"mesh": True, "model": "smpl", "ball": True})
        if name == "ball_boxes":
            ang = np.random.default_rng(11).uniform(0, 2 * np.pi, size=4)
            poses = np.stack([np.r_[-0.15 + 0.75 * np.cos(a), -0.05 + 0.75 * np.sin(a), 0.3 + 0.45 * k, 1, 0, 0, 0] for k, a in enumerate(ang)])
            m = add_free_bodies(m, [box_triangles(0.15, 0.15, 0.15)] * 4, poses, density=5.0 / 0.027, friction=1.0, condim=1)
        return dataclasses.replace(m, solver=1), make_ctrl(base, action_type="torque", residual_force=False, meta_pd=False, tq_mul=4)
    if name == "rounded":
        from tests.test_gpu_rounded_hulls import foot_model
        m = foot_model()
        return m, passive_ctrl(m)
    assert name == "chain32"
    m = caterpillar_model()
    return m, passive_ctrl(m)


def build_probe():
    """uhc_plan.cpp + tests/plan_probe.cpp -> uhc_amd/csrc/build/plan_probe.so with the host compiler: no hipcc, no HIP runtime (the HIP headers only for the struct
    definitions of uhc_device.h)."""
    return probe_build.build_probe("plan_probe.so", ["tests/plan_probe.cpp", "uhc_amd/csrc/uhc_plan.cpp"],
                                   ["uhc_amd/csrc/" + h for h in ("uhc_plan.h", "uhc_host.h", "uhc_device.h", "uhc_step_words.h")] + ["include/uhc_amd.h"], probe_build.HIP_STRUCT_FLAGS)


class Probe:
    def __init__(self, so):
        L = self.L = C.CDLL(so)
        L.uhc_plan_probe_error.restype = L.uhc_plan_probe_word_names.restype = L.uhc_plan_probe_table_names.restype = C.c_char_p
        L.uhc_plan_probe_table.restype = C.c_longlong
        L.uhc_plan_probe_table.argtypes = [C.c_char_p, C.POINTER(C.c_uint64), C.c_void_p, C.c_longlong]

    def plan(self, model, ctrl, n_env, knobs=""):
        """-> (words {name: int}, tables {name: (bytes, hash hex)})"""
        from uhc_amd._capi import model_desc
        d = model_desc(model)
        if self.L.uhc_plan_probe(C.byref(d), int(n_env), C.byref(ctrl), knobs.replace(" ", "").encode()) != 0:
            raise RuntimeError(self.L.uhc_plan_probe_error().decode())
        names = self.L.uhc_plan_probe_word_names().decode().strip(",").split(",")
        vals = (C.c_int64 * len(names))()
        assert self.L.uhc_plan_probe_words(vals, len(names)) == len(names)
        tables = {}
        for t in self.L.uhc_plan_probe_table_names().decode().strip(",").split(","):
            h = C.c_uint64(0)
            n = self.L.uhc_plan_probe_table(t.encode(), C.byref(h), None, 0)
            tables[t] = (int(n), f"{h.value:016x}")
        return dict(zip(names, [int(v) for v in vals])), tables

    def table(self, name, dtype):
        n = self.L.uhc_plan_probe_table(name.encode(), None, None, 0)
        buf = np.zeros(max(n, 1), dtype=np.uint8)
        self.L.uhc_plan_probe_table(name.encode(), None, buf.ctypes.data_as(C.c_void_p), n)
        return buf[:n].view(dtype)

    def sticky(self, inp):
        a, o = (C.c_int * 17)(*inp), (C.c_int * 10)()
        self.L.uhc_plan_probe_sticky(a, o)
        return [int(x) for x in o]

    def wiring(self, inp, n_substeps, fast_chunk, off_at_head=None):
        """off_at_head: the queues_off the step began with, which the list kernel's launch4 was decided from (default: inp's, the step's back-off did not flip)
        -> (sticky sizes {name: int}, the fast tier's chunks {name: int}, the step's launches [{field: int or None}] in launch order)"""
        nw = len(WIRING_FIELDS)
        a, o = (C.c_int * 20)(*inp, n_substeps, fast_chunk, inp[10] if off_at_head is None else off_at_head), (C.c_int * (15 + 4 * nw))()
        self.L.uhc_plan_probe_wiring(a, o)
        o = [int(x) for x in o]
        launches = [dict(zip(WIRING_FIELDS, o[15 + nw * k:15 + nw * (k + 1)])) for k in range(o[14])]
        for l in launches:
            for f in WIRING_SLOTS:
                l[f] = None if l[f] == -1 else l[f]  # UHC_NONE
        return dict(zip(STICKY_OUT, o[:10])), dict(zip(("chunk", "n_chunks", "grid", "prod_total"), o[10:14])), launches


STICKY_OUT = ("queues", "waiting", "q3", "q4", "launch4", "grid2", "grid3", "grid4", "n_wait", "sticky_mask")
# StepLaunch (uhc_plan.h) in the order of its declaration; the fields that hold a slot of the batch's lists / counts / cursors / fin, or none
WIRING_FIELDS = ("tier", "stream", "list", "count", "cursor", "grid", "n_wait", "spares", "started", "prod_fin", "prod_total", "fin", "next_list", "next_count",
                 "gate_started", "gate_want", "gate_waited", "tier_want", "chunk", "use_order")
WIRING_SLOTS = ("list", "count", "cursor", "spares", "started", "prod_fin", "fin", "next_list", "next_count", "gate_started", "gate_waited")
SLOT = {k: int(v) for k, v in re.findall(r"\b(UHC_[A-Z0-9_]+) = (\d+)", open(os.path.join(CSRC, "uhc_device.h")).read())}  # the enumerators the list kernel indexes by
N_WORDS, N_LISTS = int(re.search(r"#define UHC_N_WORDS (\d+)", open(os.path.join(CSRC, "uhc_device.h")).read()).group(1)), SLOT["UHC_N_LISTS"]  # ints allocated for counts / cursors / fin; env queues
# what uhc_tier_lists_kernel fills for each tier's consumers: (list, count, cursor)
QUEUE_OF_TIER = {2: ("UHC_LIST_GEN", "UHC_CNT_GEN", "UHC_CUR_GEN"), 3: ("UHC_LIST_BIG", "UHC_CNT_BIG", "UHC_CUR_BIG"), 4: ("UHC_LIST_T4", "UHC_CNT_T4", "UHC_CUR_T4")}


@pytest.fixture(scope="module")
def probe():
    return Probe(build_probe())


@pytest.fixture(scope="module")
def recording():
    return json.load(open(RECORDING))


_models = {}


def _class(name):
    if name not in _models:
        _models[name] = model_class(name)
    return _models[name]


def case_key(cls, n_env, knobs):
    return f"{cls}|{n_env}|{knobs}"


ALL_CASES = [(c, n, "") for c in CLASSES for n in N_ENVS] + [("generated", n, k) for k in KNOB_CASES for n in N_ENVS]


# ---------------------------------------------------------------------------------------------------------------- a. invariants
def _primal_scratch_total(nv, YS):  # uhc_device.h primal_scratch
    o = 0
    for n in ((nv * YS + 3) // 4 + 1, 4 * 16 * 32, nv * 8, 528 // 4, 4 * 144 // 4, (4 * 33 + 3) // 4, 4 * 32, 4, 4 * 128, 1024 // 2):
        o += (n + 1) & ~1
    return o


def _regions(W, tier):
    """-> (persistent + constraint-phase regions {name: (offset, doubles)}, phase-1 overlays {name: (offset, doubles)}) of layout `tier` (0 fast, 1 general, 2 large, 3 tier 4)"""
    lp, cp = ("lf.", "l.", "lh.", "lx.")[tier], ("cf.", "cg.", "ch.", "cx.")[tier]
    nq, nv, nu, nb, nj, nM = (W["t." + k] for k in ("nq", "nv", "nu", "nbody", "njnt", "nM"))
    YS, nvp, dense_model = W["t.maxdepth"] + 1, W["nvp"], W["t.ncpair"] > 0
    maxefc, maxcon, ndense, ycap = (W[cp + k] for k in ("maxefc", "maxcon", "ndense", "ycap"))
    fast, huge = tier == 0, tier == 3 and W["last_tier"] == 4
    size = dict(qpos=nq, qvel=nv, qacc=nv, ctrl=nu, applied=nv, bias=nv, smooth=nv, z=nv, dinv=nv, sdinv=nv, zero=2, LD=nM + 2, cdof=6 * nv,
                xpos=3 * nb, xquat=4 * nb, xmat=9 * nb, xipos=3 * nb, rootcom=3 * nb)
    if fast and not dense_model:
        size["mij"] = (nM + 3) // 4 + 1
    if not fast:
        size["vec"] = nv
    if fast:
        size.update(con=maxcon * 24, rowMisc=128, ncon_nefc=2 + 32 // 2, dense=ndense * nvp, Y=ycap)
        if W[lp + "dcol"] != W[lp + "con"]:
            size["dcol"] = ndense * 64
    elif huge:
        size.update(con=max(maxcon * 24, _primal_scratch_total(nv, YS)), rowMisc=max(maxefc * 2, 128), ncon_nefc=2 + (ndense + 1) // 2 + 1, rowY=maxefc // 2 + 1,
                    dsc=max(ndense * 4, 2), H=nv * (nv + 1) // 2)
    else:
        size.update(con=max(maxcon * 24, ndense * 64), rowMisc=maxefc * 2, ncon_nefc=2 + 32, rowY=maxefc // 2 + 1, dense=ndense * nvp, dsc=ndense * 4, Y=ycap)
    if not fast:
        size.update({k: maxefc for k in ("rowR", "rowAref", "rowB", "rowF", "rowDa", "rowW")})
    phase1 = dict(cinert=10 * nb, ximat=9 * nb, xanchor=3 * nj, xaxis=3 * nj, cdofdot=6 * nv, crb=10 * nb, cvel=6 * nb, cacc=6 * nb, cfrc=6 * nb)
    return ({k: (W[lp + k], n) for k, n in size.items() if n > 0}, {k: (W[lp + k], n) for k, n in phase1.items()})


def _tiers(W):
    return [0, 1] + ([2, 3] if W["last_tier"] >= 3 else [])


def _hinge_only(model):
    return not any(int(t) == 1 for t in model.jnt_type)  # UHC_JNT_BALL


@pytest.mark.parametrize("cls,n_env,knobs", ALL_CASES, ids=[case_key(*c) for c in ALL_CASES])
def test_layout_invariants(probe, cls, n_env, knobs):
    model, ctrl = _class(cls)
    W, _ = probe.plan(model, ctrl, n_env, knobs)
    guard = probe.table("guard_tab", np.int32) if "UHC_GUARD_LDS=1" in knobs else None
    assert guard is None or guard.size == 4 * 64
    for t in _tiers(W):
        lp, cp = ("lf.", "l.", "lh.", "lx.")[t], ("cf.", "cg.", "ch.", "cx.")[t]
        total = W[lp + "total"]
        regs, over = _regions(W, t)
        for k, (o, n) in list(regs.items()) + list(over.items()):
            assert o % 2 == 0 and o >= 0, f"tier {t}: offset of {k} = {o}"
            assert o + n <= total, f"tier {t}: {k} [{o}, {o + n}) ends beyond total {total}"
        spans = sorted((o, o + n, k) for k, (o, n) in regs.items())
        for (a0, a1, ka), (b0, b1, kb) in zip(spans, spans[1:]):
            assert a1 <= b0, f"tier {t}: {ka} [{a0}, {a1}) overlaps {kb} [{b0}, {b1})"
        assert total * 8 <= 160 * KIB
        assert 2 * regs["rowMisc"][1] >= 256  # before the rows are enumerated the region is the collision stage's candidate list: CAND_CAP = 256 ints (uhc_physics_impl.h)
        vs, huge = W[cp + "vstage"], t == 3 and W["last_tier"] == 4
        assert vs == -1 or vs == W[lp + ("H" if huge else "dense")]  # the dense rows (+ Yhat behind them) / tier 4: where the Hessian will be
        if guard is not None:
            g = guard[64 * t:64 * t + 64]
            words = list(g[2:2 + g[0]]) + list(g[32:32 + g[1]])
            assert g[0] > 0 and g[1] > 0
            for gw in words:
                assert gw % 2 == 0 and gw + 2 <= total
                for a0, a1, k in spans:
                    assert gw + 2 <= a0 or gw >= a1, f"tier {t}: guard word at {gw} inside {k} [{a0}, {a1})"
    if W["last_tier"] >= 3:
        assert 2 * W["l.total"] * 8 <= 160 * KIB  # two general-tier workgroups per CU
    assert W["lds_bytes"] == W["l.total"] * 8 and W["lds_bytes_fast"] == W["lf.total"] * 8
    # the fast layout: 40 KiB, four per CU (one per SIMD); with body-body rows 52 KiB, three per CU -- from 3072 envs on a hinge-only humanoid without objects gets the 40 KiB one too
    fits = (160 * KIB) // W["lds_bytes_fast"]
    if "UHC_FAST_DENSE" in knobs:
        assert W["lds_bytes_fast"] <= 40 * KIB and fits == 4
    elif W["t.ncpair"] == 0 or (n_env >= 3072 and _hinge_only(model) and W["n_trailing_free"] == 0):
        assert W["lds_bytes_fast"] <= 40 * KIB and fits == 4
    else:
        assert 40 * KIB < W["lds_bytes_fast"] <= 52 * KIB and fits == 3
    # the schedules' 16-bit LDS byte addresses: the fast layout's LD buffer, and the general tier's (its own LD offset added to them)
    nM = W["t.nM"]
    assert W["lf.LD"] * 8 + 8 * (nM + 1) + 8 <= 65536 and W["l.LD"] * 8 + 8 * (nM + 2) <= 65536
    lo, hi = W["lf.LD"] * 8, W["lf.LD"] * 8 + 8 * (nM + 2)
    for name in ("fac_prog", "sol_back", "sol_fwd"):
        a = probe.table(name, np.uint32)
        if name == "fac_prog":
            a = a.reshape(-1, 6)[:, :5]  # (the sixth word of a record is one address: D_k)
            assert np.all((probe.table(name, np.uint32).reshape(-1, 6)[:, 5] >= lo) & (probe.table(name, np.uint32).reshape(-1, 6)[:, 5] < hi))
        for half in (a & 0xffff, a >> 16):
            assert np.all((half >= lo) & (half < hi)), name
    ch = probe.table("chain", np.uint32) >> 16
    assert np.all((ch >= lo) & (ch < hi))
    for t in (1, 2, 3):
        if t in _tiers(W):
            assert W[("cg.", "ch.", "cx.")[t - 1] + "ld_delta"] == (W[("l.", "lh.", "lx.")[t - 1] + "LD"] - W["lf.LD"]) * 8
    # the marks follow the fast layout unless UHC_TIER_MARKS names them
    m = [W[f"marks{k}"] for k in range(8)]
    if "UHC_TIER_MARKS" in knobs:
        assert m == [int(x) for x in knobs.split("=")[1].split(",")]
    else:
        nd, mc = W["cf.ndense"], W["cf.maxcon"]
        assert m == [64, mc, nd if nd > 0 else 12, 56, mc - max(2, mc // 8), (max(1, nd - (2 if nd > 8 else 1)) if nd > 0 else 10), 8, 7]


def test_sticky_step_invariants(probe):
    for inp in sticky_inputs():
        o = dict(zip(STICKY_OUT, probe.sticky(inp)))
        n_env, q4_max = inp[5], inp[15]
        assert not o["queues"] or o["grid2"] > 0, inp
        assert not o["q3"] or o["grid3"] > 0, inp
        assert not o["q4"] or o["grid4"] > 0, inp
        assert o["grid2"] <= n_env, inp
        assert o["grid4"] <= q4_max, inp
        assert o["sticky_mask"] == 4 * o["queues"] + 8 * o["q3"] + 16 * o["launch4"]


def wiring_cases():
    """(inputs, queues_off at the head of the step): the sticky grid; the same with three and two tiers (no tier 4; no large tier either); and the step in which the
    back-off flips -- launch4 decided while the queues were still on, the sizes planned with them off."""
    grid = sticky_inputs()
    cases = [(inp, inp[10]) for inp in grid]
    for last_tier in (3, 2):
        cases += [(inp[:9] + [last_tier] + inp[10:], inp[10]) for inp in grid]
    return cases + [(inp, 0) for inp in grid if inp[10] == 1]


@pytest.mark.parametrize("n_substeps,fast_chunk", [(0, 0), (15, 0), (15, 3), (15, 5), (15, 15)])
def test_sticky_wiring_invariants(probe, n_substeps, fast_chunk):
    """The step's table of launches (sticky_wiring): every invariant between a queue's producers and its consumers, whatever the sizes, and the queue each tier's
    consumers read is the one the list kernel fills for that tier."""
    for inp, off_at_head in wiring_cases():
        z, fast, launches = probe.wiring(inp, n_substeps, fast_chunk, off_at_head)
        n_env, large_first, last_tier = inp[5], inp[8], inp[9]
        by_tier = {l["tier"]: l for l in launches}
        assert len(by_tier) == len(launches), inp
        consumers = [l for l in launches if l["list"] is not None]
        for l in consumers:
            assert (l["list"], l["count"], l["cursor"]) == tuple(SLOT[k] for k in QUEUE_OF_TIER[l["tier"]]), inp
        assert (3 in by_tier) == bool(z["queues"] and last_tier >= 3) and (last_tier == 4 or 4 not in by_tier), inp
        assert z["launch4"] == (last_tier == 4 and inp[2] > 0 and inp[3] > 0 and not off_at_head), inp  # sticky_launch4 of what the step began with
        # which launches the step has, and the mask the kernels filter by
        assert set(by_tier) == {1} | ({2} if z["queues"] else set()) | ({3} if z["q3"] else set()) | ({4} if z["q4"] else set()), inp
        assert z["sticky_mask"] == 4 * (2 in by_tier) + 8 * (3 in by_tier) + 16 * z["launch4"], inp
        assert (4 in by_tier) == bool(z["launch4"] and 3 in by_tier), inp
        # the order: tier 4 first, large before general exactly when large_first, the fast tier last
        want = [t for t in ([4, 3, 2] if large_first else [4, 2, 3]) if t in by_tier] + [1]
        assert [l["tier"] for l in launches] == want, inp
        assert [l["stream"] for l in launches] == [{1: 0, 2: 1, 3: 2, 4: 3}[t] for t in want], inp  # the batch's stream; a side stream per tier
        # the fast tier's launch
        f = by_tier[1]
        assert f["list"] is None and f["count"] is None and f["cursor"] is None and f["tier_want"] == 1 and f["use_order"] == 1, inp
        assert f["chunk"] == fast["chunk"] and f["grid"] == fast["grid"] == fast["n_chunks"] * n_env, inp
        assert (f["chunk"] == 0) == (fast["n_chunks"] == 1), inp
        assert (f["fin"] is not None) == (f["next_list"] is not None) == (f["next_count"] is not None) == bool(z["waiting"]), inp
        for l in consumers:
            assert l["list"] is not None and l["count"] is not None and l["cursor"] is not None and l["grid"] > 0, inp
            assert l["tier_want"] == 0 and l["chunk"] == 0 and l["use_order"] == 0, inp
            assert l["grid"] == {2: z["grid2"], 3: z["grid3"], 4: z["grid4"]}[l["tier"]], inp
        # producers: a consumer waits for the exits of a launch of this step, all of them
        for l in consumers:
            if l["prod_fin"] is None:
                assert l["prod_total"] == 0, inp
                continue
            prod = [p for p in launches if p["fin"] == l["prod_fin"]]
            assert len(prod) == 1 and prod[0] is not l, inp
            assert l["prod_total"] == prod[0]["grid"], inp
        # hand-ons: into the queue of a consumer launch of this step, and only from the tier directly below it
        for l in launches:
            assert (l["next_list"] is None) == (l["next_count"] is None), inp
            if l["next_list"] is not None:
                into = [c for c in consumers if (c["list"], c["count"]) == (l["next_list"], l["next_count"])]
                assert len(into) == 1 and into[0]["tier"] == l["tier"] + 1, inp
                assert into[0]["prod_fin"] == l["fin"] and l["fin"] is not None, inp  # whoever appends to a queue is waited for by its consumers
        # gates: for a consumer launch of this step to be resident, all of it
        for l in launches:
            if l["gate_started"] is None:
                assert l["gate_want"] == 0 and l["gate_waited"] is None, inp
                continue
            behind = [c for c in consumers if c["started"] == l["gate_started"]]
            assert len(behind) == 1 and l["gate_want"] == behind[0]["grid"], inp
            assert launches.index(behind[0]) < launches.index(l), inp
        if 2 in by_tier:
            assert (by_tier[2]["gate_started"] is not None) == bool(3 in by_tier and large_first), inp
        assert (f["gate_started"] is not None) == bool(z["waiting"]), inp
        assert all(by_tier[t]["gate_started"] is None for t in (3, 4) if t in by_tier), inp
        # no slot is shared, none lies beyond the allocation
        for field, room in (("list", N_LISTS), ("count", N_WORDS), ("cursor", N_WORDS)):
            used = [l[field] for l in consumers] + ([l["gate_waited"] for l in launches if l["gate_waited"] is not None] if field == "count" else [])
            assert len(set(used)) == len(used) and all(0 <= u < room for u in used), (field, inp)
        fins = [l[k] for l in launches for k in ("fin", "started", "spares") if l[k] is not None]
        assert len(set(fins)) == len(fins) and all(0 <= u < N_WORDS for u in fins), inp
        for l in launches:
            for k in ("prod_fin", "gate_started"):
                assert l[k] is None or 0 <= l[k] < N_WORDS, inp
            assert l["next_list"] is None or (0 <= l["next_list"] < N_LISTS and 0 <= l["next_count"] < N_WORDS), inp
        # who waits on an empty queue: the general tier's consumers share a seat counter, every other consumer waits
        for l in consumers:
            if l["tier"] == 2:
                assert l["spares"] is not None and l["n_wait"] == z["n_wait"], inp
            else:
                assert l["spares"] is None and l["n_wait"] == l["grid"], inp
        assert f["spares"] is None and f["n_wait"] == 0 and f["started"] is None and f["prod_fin"] is None, inp


# ---------------------------------------------------------------------------------------------------------------- b. equality with the recording
@pytest.mark.parametrize("cls,n_env,knobs", ALL_CASES, ids=[case_key(*c) for c in ALL_CASES])
def test_plan_equals_the_recording(probe, recording, cls, n_env, knobs):
    model, ctrl = _class(cls)
    W, tables = probe.plan(model, ctrl, n_env, knobs)
    rec = recording["plans"][case_key(cls, n_env, knobs)]
    want = dict(zip(recording["word_names"], rec["words"]))
    assert set(W) == set(want)
    diff = {k: (W[k], want[k]) for k in W if W[k] != want[k]}
    assert not diff, f"plan words differ from the recording (now, recorded): {diff}"
    assert {k: list(v) for k, v in tables.items()} == rec["tables"]


def test_sticky_step_equals_the_recording(probe, recording):
    inputs = sticky_inputs()
    assert len(inputs) == len(recording["sticky"]) == 6 * 4 * 3 * 2 * 2 * 2
    for inp, want in zip(inputs, recording["sticky"]):
        assert probe.sticky(inp) == want, inp
