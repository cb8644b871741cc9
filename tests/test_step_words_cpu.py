"""The step's status words and the tier policy on the CPU: uhc_amd/csrc/uhc_step_words.h (plain integer code the kernels inline) compiled with the host compiler
into the plan probe (tests/plan_probe.cpp) and fed the PLANNED marks and capacities of the model classes tests/test_batch_plan_cpu.py builds.

a. Equality with tests/step_words_recording.json: what the expressions of the commit before this header existed -- lifted verbatim out of uhc_step_env, k_forward
   and uhc_tier_lists_kernel into a host program -- gave on the grid below (recorded once; the grid is regenerated here, the recording holds the plans' marks and
   capacities and the outputs).  Every tier against every last_tier runs on ONE plan's marks (SWEEP_LAST_TIER); the other five plans run every tier against
   their own last_tier -- 2 and 3 among them (UHC_TIERS).
b. Invariants nothing else states: where each status bit lands in UHC_F_REDO, the hysteresis of the tiers, monotonicity of the policy, the fresh env's place,
   the chunk record's merge.
c. include/uhc_amd.h's UHC_REDO_* / UHC_HANDON_* against uhc_amd/sim.py's REDO_* / WHY_*; its UHC_DEBUG_* / UHC_TRACE_* against DEBUG_* / TRACE_*."""
import ctypes as C
import itertools
import json
import os
import re

import pytest

from tests.test_batch_plan_cpu import Probe, build_probe, model_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDING = os.path.join(ROOT, "tests", "step_words_recording.json")
N_ENV = 1024
PLANS = (("asset", ""), ("generated", ""), ("ball_boxes", ""), ("generated", "UHC_TIER_MARKS=60,20,10,50,16,8,8,6"), ("generated", "UHC_TIERS=2"), ("generated", "UHC_TIERS=3"))
SWEEP_LAST_TIER = ("generated", "")  # the plan whose grid runs every tier against every last_tier (the others: their own)
T4_ROWS = 96
NAMES = ("ST_HANDON", "ST_DROPPED", "ST_SWEPT", "ST_WHY_FRICTION", "ST_WINDOWED", "ST_WHY_NOCONV", "ST_WHY_PIVOT", "ST_PRIMAL", "ST_PRIMAL_CAP", "WHY_SHIFT",
         "WS_FRICTION", "WS_LOST", "WS_NOCONV", "WS_PIVOT", "WS_TIER4", "REC_PK_NEFC", "REC_PK_NCON", "REC_PK_NTWO", "REC_PK_Y", "REC_PK_ACT", "REC_NCON", "REC_NEFC",
         "REC_ITERS", "REC_STATUS", "CHUNK_REC", "ORDER_BUCKETS")
STATUS = NAMES[:9]
BUCKET_EDGES = (24, 40, 48, 52, 56, 59, 62)


class Words:
    """the probe's uhc_sw_* entry points (tests/plan_probe.cpp); `plan` first: next_tier and launch_cost read the marks and capacities of the plan probed last"""

    def __init__(self, probe):
        self.probe, self.L = probe, probe.L
        self.L.uhc_sw_launch_cost.argtypes = [C.POINTER(C.c_int), C.c_double]
        n = (C.c_int * len(NAMES))()
        self.L.uhc_sw_names(n)
        self.K = dict(zip(NAMES, [int(x) for x in n]))

    def plan(self, cls, knobs):
        model, ctrl = _class(cls)
        W, _ = self.probe.plan(model, ctrl, N_ENV, knobs)
        return W

    def next_tier(self, tier, pk, last_tier=-1, t4_rows=-1, sticky4=0):
        return int(self.L.uhc_sw_next_tier(tier, (C.c_int * 5)(*pk), last_tier, t4_rows, sticky4))

    def launch_cost(self, pk, vmax_end):
        return int(self.L.uhc_sw_launch_cost((C.c_int * 5)(*pk), float(vmax_end)))

    def redo_word(self, tier, status, swept):
        return int(self.L.uhc_sw_redo_word(tier, status, swept))

    def redo_written(self, tier, status):
        return bool(self.L.uhc_sw_redo_written(tier, status))

    def swept_mask(self, mask, status, it):
        return int(self.L.uhc_sw_swept_mask(mask, status, it))

    def ws_gave_up_status(self, exact, code):
        return int(self.L.uhc_sw_ws_gave_up_status(exact, code))

    def handon_why_word(self, tier, old, status, substep):
        return int(self.L.uhc_sw_handon_why_word(tier, old, status, substep)) & 0xffffffff

    def order_bucket(self, tier, masked, active, fresh, cost):
        return int(self.L.uhc_sw_order_bucket(tier, masked, active, fresh, cost))

    def start_tier(self, tier, fresh, launch4):
        return int(self.L.uhc_sw_start_tier(tier, fresh, launch4))

    def chunk_rec_merge(self, pk, status, rec):
        p, s = (C.c_int * 5)(*pk), C.c_int(status)
        self.L.uhc_sw_chunk_rec_merge(p, C.byref(s), (C.c_int * len(rec))(*rec))
        return [int(x) for x in p], int(s.value)


_models = {}


def _class(name):
    if name not in _models:
        _models[name] = model_class(name)
    return _models[name]


@pytest.fixture(scope="module")
def words():
    return Words(Probe(build_probe()))


@pytest.fixture(scope="module")
def recording():
    return json.load(open(RECORDING))


def plan_key(cls, knobs):
    return f"{cls}|{N_ENV}|{knobs}"


# ---------------------------------------------------------------------------------------------------------------- the grid
PEAKS = ("nefc", "ncon", "ntwo", "y", "act")
ARG_WORDS = tuple(f"marks{k}" for k in range(8)) + tuple(f"{c}.{k}" for c in ("cf", "cg", "ch") for k in ("maxefc", "maxcon", "ndense", "ycap")) + ("last_tier", "t4_rows")


def thresholds(W):
    """-> {peak: the values at which some comparison of next_tier flips}: the marks; the eighths of the general tier's capacities, (m cap) // 8 -- the value and
    the one above it are the two sides of the integer division; the packed storage's 7/8 of the fast tier's, less the slack of 8"""
    m = [W[f"marks{k}"] for k in range(8)]
    e = lambda k, cap: (m[k] * W["cg." + cap]) // 8
    return dict(nefc=[m[0], m[3], e(6, "maxefc"), e(7, "maxefc")], ncon=[m[1], m[4], e(6, "maxcon"), e(7, "maxcon")], ntwo=[m[2], m[5], e(6, "ndense"), e(7, "ndense")],
                y=[(7 * W["cf.ycap"]) // 8 - 8, e(6, "ycap"), e(7, "ycap")])


def peak_cases(W):
    """zero; each peak at each of its thresholds, one below and one above, the others zero; all peaks together at the up2 / dn1 / up3 / dn2 thresholds and one off"""
    th = thresholds(W)
    out = [[0, 0, 0, 0, 0]]
    for k, name in enumerate(PEAKS[:4]):
        for v in th[name]:
            for d in (-1, 0, 1):
                pk = [0, 0, 0, 0, 0]
                pk[k] = max(v + d, 0)
                out.append(pk)
    for j in range(4):  # up2, dn1, up3, dn2 (y has no up2 mark: its dn1 threshold twice)
        for d in (-1, 0, 1):
            out.append([max(th["nefc"][j] + d, 0), max(th["ncon"][j] + d, 0), max(th["ntwo"][j] + d, 0), max(th["y"][max(j - 1, 0)] + d, 0), 0])
    return out


def next_tier_cases(W, sweep):
    """-> [(tier, peaks, last_tier, t4_rows, sticky4)]"""
    out = [(t, pk, lt, 0, 0) for lt in ((2, 3, 4) if sweep else (W["last_tier"],)) for t in (1, 2, 3, 4) for pk in peak_cases(W)]
    # the tier-4 row mark: none and a mid value, the peak rows at the mark, at 3/4 of it, and one off each
    for rows in (0, T4_ROWS):
        for lt in (3, 4):
            for t in (1, 2, 3, 4):
                out += [(t, [n, 0, 0, 0, 0], lt, rows, 0) for n in (T4_ROWS - 1, T4_ROWS, T4_ROWS + 1, (3 * T4_ROWS) // 4 - 1, (3 * T4_ROWS) // 4, (3 * T4_ROWS) // 4 + 1)]
    # the measurement switch's release from tier 4: 3/4 of the large tier's capacities, 48 force-carrying rows
    q = [(3 * W["ch." + c]) // 4 for c in ("maxefc", "maxcon", "ndense")] + [0, 48]
    for k in (0, 1, 2, 4):
        for d in (0, 1):
            pk = list(q)
            pk[k] += d
            out += [(4, pk, 4, 0, s4) for s4 in (0, 1)]
    return out


def cost_cases(W):
    together = [W["marks0"], W["marks1"], W["marks2"], (7 * W["cf.ycap"]) // 8, 0]
    return [(pk, 0.0) for pk in peak_cases(W)] + [(pk, v) for pk in ([0, 0, 0, 0, 0], together, [30, 2, 1, 100, 0]) for v in (0.0, 30.0, 30.0 + 1e-9, 60.0, 60.0 + 1e-9)]


def bucket_cases():
    costs = sorted({0, 64, 100} | set(BUCKET_EDGES) | {c - 1 for c in BUCKET_EDGES})
    return [(t, m, a, f, c) for t in (1, 2, 3, 4) for m, a in ((0, 0), (1, 0), (1, 1)) for f in (0, 1) for c in (costs if t == 1 else (0, 30, 64))]


def start_cases():
    return list(itertools.product((1, 2, 3, 4), (0, 1), (0, 1)))


def redo_cases(K):
    bits = [K[n] for n in STATUS] + [1 << K["WHY_SHIFT"], 1 << (K["WHY_SHIFT"] + 5)]
    combos = [0, K["ST_SWEPT"] | K["ST_WHY_FRICTION"], K["ST_SWEPT"] | K["ST_WHY_NOCONV"] | K["ST_DROPPED"], K["ST_SWEPT"] | K["ST_WHY_PIVOT"] | K["ST_WINDOWED"],
              K["ST_PRIMAL"] | K["ST_PRIMAL_CAP"], K["ST_PRIMAL"] | K["ST_SWEPT"] | K["ST_WHY_FRICTION"] | K["ST_DROPPED"], sum(K[n] for n in STATUS)]
    swept = [0, 1 << 8, 1 << 28, ((1 << 21) - 1) << 8, (1 << 8) | (1 << 22)]
    return [(t, s, w) for t in (1, 2, 3, 4) for s in bits + combos for w in swept]


def why_cases(K):
    sh = K["WHY_SHIFT"]
    statuses = [(1 << (sh + k)) | K["ST_HANDON"] for k in range(6)] + [(0x3f << sh) | K["ST_HANDON"], (0x05 << sh) | K["ST_HANDON"] | K["ST_DROPPED"], K["ST_HANDON"]]
    return [(t, old, s, it) for t in (1, 2, 3, 4) for old in (0x2a0d1103, 0) for s in statuses for it in (0, 7, 14, 255, 300)]


def merge_cases(K):
    rec0 = [0] * K["CHUNK_REC"]
    rec1 = [40, 9, 3, 700, 12, 5, 33, 4, K["ST_DROPPED"]] + [0] * (K["CHUNK_REC"] - 9)
    rec2 = [10, 20, 0, 50, 0, 1, 2, 3, 0] + [77] * (K["CHUNK_REC"] - 9)
    return [(pk, s, r) for pk in ([0, 0, 0, 0, 0], [40, 9, 3, 700, 12], [41, 2, 7, 10, 30]) for s in (0, K["ST_DROPPED"]) for r in (rec0, rec1, rec2)]


def outputs(words, with_args=True):
    """-> the whole grid's outputs in the recording's layout"""
    K = words.K
    out = {"plans": {}}
    for cls, knobs in PLANS:
        W = words.plan(cls, knobs)
        out["plans"][plan_key(cls, knobs)] = dict(
            args=[W.get(k, 0) for k in ARG_WORDS],
            next_tier="".join(str(words.next_tier(*c)) for c in next_tier_cases(W, (cls, knobs) == SWEEP_LAST_TIER)),
            cost=[words.launch_cost(*c) for c in cost_cases(W)])
    out["order_bucket"] = "".join(str(words.order_bucket(*c)) for c in bucket_cases())
    out["start_tier"] = "".join(str(words.start_tier(*c)) for c in start_cases())
    out["redo_word"] = [words.redo_word(*c) for c in redo_cases(K)]
    out["swept_mask"] = [words.swept_mask(m, s, it) for m in (0, 1 << 9) for s in (0, K["ST_SWEPT"], K["ST_SWEPT"] | K["ST_WHY_PIVOT"], K["ST_DROPPED"]) for it in range(-2, 24)]
    out["ws_gave_up_status"] = [words.ws_gave_up_status(x, c) for x in (0, 1) for c in (-1, -2, -3, -4)]
    out["handon_why_word"] = [words.handon_why_word(*c) for c in why_cases(K)]
    out["chunk_rec_merge"] = [list(words.chunk_rec_merge(*c)) for c in merge_cases(K)]
    return out


# ---------------------------------------------------------------------------------------------------------------- a. equality with the recording
def test_policy_and_words_equal_the_recording(words, recording):
    got = outputs(words)
    assert set(got) == set(recording) and set(got["plans"]) == set(recording["plans"])
    for key, want in recording["plans"].items():
        g = got["plans"][key]
        assert g["args"] == want["args"], f"{key}: the plan's marks / capacities are not the recorded ones"
        assert len(g["next_tier"]) == len(want["next_tier"]) and len(g["cost"]) == len(want["cost"]), key
        cls, knobs = key.split("|")[0], key.split("|")[2]
        W = dict(zip(ARG_WORDS, g["args"]))
        bad = [(c, a, b) for c, a, b in zip(next_tier_cases(W, (cls, knobs) == SWEEP_LAST_TIER), g["next_tier"], want["next_tier"]) if a != b]
        assert not bad, f"{key}: next_tier differs from the recording (case, now, recorded): {bad[:5]}"
        bad = [(c, a, b) for c, a, b in zip(cost_cases(W), g["cost"], want["cost"]) if a != b]
        assert not bad, f"{key}: launch_cost differs from the recording (case, now, recorded): {bad[:5]}"
    for name in ("order_bucket", "start_tier", "redo_word", "swept_mask", "ws_gave_up_status", "handon_why_word", "chunk_rec_merge"):
        assert got[name] == recording[name], name


def test_the_grid_covers_what_it_claims(words):
    K = words.K
    W = words.plan(*SWEEP_LAST_TIER)
    cases = next_tier_cases(W, True)
    assert {(c[0], c[2]) for c in cases} >= set(itertools.product((1, 2, 3, 4), (2, 3, 4)))
    assert {c[3] for c in cases} == {0, T4_ROWS} and {c[4] for c in cases} == {0, 1}
    assert {v for _, v in cost_cases(W)} == {0.0, 30.0, 30.0 + 1e-9, 60.0, 60.0 + 1e-9}
    assert {c[4] for c in bucket_cases() if c[0] == 1} >= set(BUCKET_EDGES) | {e - 1 for e in BUCKET_EDGES}
    assert {c[1] for c in redo_cases(K)} >= {K[n] for n in STATUS}
    # the bucket edges of the grid are the ones order_bucket's chain names
    src = open(os.path.join(ROOT, "uhc_amd", "csrc", "uhc_step_words.h")).read()
    assert tuple(sorted(int(x) for x in re.findall(r"c >= (\d+) \?", src))) == BUCKET_EDGES


# ---------------------------------------------------------------------------------------------------------------- b. invariants
def _public():
    from uhc_amd import sim as S
    return S


def test_redo_word_puts_every_status_bit_on_its_documented_bit(words):
    K, S = words.K, _public()
    where = {"ST_HANDON": 0, "ST_DROPPED": S.REDO_DROPPED, "ST_SWEPT": S.REDO_SWEPT, "ST_WHY_FRICTION": S.REDO_WHY_FRICTION, "ST_WINDOWED": S.REDO_WINDOWED,
             "ST_WHY_NOCONV": S.REDO_WHY_NOCONV, "ST_WHY_PIVOT": S.REDO_WHY_PIVOT, "ST_PRIMAL": S.REDO_PRIMAL, "ST_PRIMAL_CAP": S.REDO_PRIMAL_CAP}
    assert len({K[n] for n in STATUS}) == len(STATUS) and all(K[n] & (K[n] - 1) == 0 for n in STATUS)
    for tier in (2, 3, 4):
        base = S.REDO_GENERAL | (S.REDO_LARGE if tier >= 3 else 0)
        assert words.redo_word(tier, 0, 0) == base
        for n in STATUS:
            assert words.redo_word(tier, K[n], 0) == base | where[n], (tier, n)
        for k in range(K["WHY_SHIFT"], 31):  # the reasons of a hand-on are not UHC_F_REDO's
            assert words.redo_word(tier, 1 << k, 0) == base
    for n in STATUS:  # the fast tier: the truncation bit alone, and nothing at all otherwise (the step's cleared word stays)
        assert words.redo_word(1, K[n], 0) == (S.REDO_DROPPED if n == "ST_DROPPED" else 0)
    for status in range(1 << len(STATUS)):  # a word is written exactly when it differs from the step's cleared one
        assert [words.redo_written(t, status) for t in (1, 2, 3, 4)] == [words.redo_word(t, status, 0) != 0 for t in (1, 2, 3, 4)] == [bool(status & K["ST_DROPPED"]), True, True, True]
    # the three reasons are k_as_general's codes, none of them the windowed bit; the code without a reason reports the sweeps alone
    gave_up = {c: words.ws_gave_up_status(1, K[c]) for c in ("WS_FRICTION", "WS_LOST", "WS_NOCONV", "WS_PIVOT")}
    assert gave_up == {"WS_FRICTION": K["ST_SWEPT"] | K["ST_WHY_FRICTION"], "WS_LOST": K["ST_SWEPT"], "WS_NOCONV": K["ST_SWEPT"] | K["ST_WHY_NOCONV"],
                       "WS_PIVOT": K["ST_SWEPT"] | K["ST_WHY_PIVOT"]}
    assert all(not (v & K["ST_WINDOWED"]) for v in gave_up.values())
    assert all(words.ws_gave_up_status(0, K[c]) == K["ST_SWEPT"] for c in gave_up)  # (solver 0: the sweeps are the solver, nothing gave up)


def test_redo_word_stays_inside_the_documented_bits(words):
    K, S = words.K, _public()
    field = sum(S.REDO_SWEPT_SUBSTEP0 << k for k in range(S.REDO_SWEPT_SUBSTEPS))
    documented = (S.REDO_GENERAL | S.REDO_SWEPT | S.REDO_WHY_FRICTION | S.REDO_WINDOWED | S.REDO_WHY_NOCONV | S.REDO_WHY_PIVOT | S.REDO_LARGE | S.REDO_DROPPED | field |
                  S.REDO_PRIMAL_CAP | S.REDO_PRIMAL)
    assert documented == 0x7fffffff and field & (S.REDO_PRIMAL | S.REDO_PRIMAL_CAP) == 0
    bits = [words.swept_mask(0, K["ST_SWEPT"], it) for it in range(-3, 40)]
    assert all(words.swept_mask(1 << 9, K["ST_SWEPT"], it) == (1 << 9) | b and words.swept_mask(1 << 9, sum(K[n] for n in STATUS) & ~K["ST_SWEPT"], it) == 1 << 9 for it, b in zip(range(-3, 40), bits))
    assert all(b & ~field == 0 and b & (b - 1) == 0 for b in bits)  # one bit of the field, or none: never bits 29 or 30
    assert [b for b in bits if b] == [S.REDO_SWEPT_SUBSTEP0 << k for k in range(S.REDO_SWEPT_SUBSTEPS)]
    every = 0
    for b in bits:
        every |= b
    assert every == field
    for tier in (1, 2, 3, 4):
        for status in range(1 << len(STATUS)):
            for why in (0, 0x3f << K["WHY_SHIFT"]):
                assert words.redo_word(tier, status | why, every) & ~documented == 0
    # the substeps the checker is told to sweep are exactly that field
    from oracle.physics import swept_substeps
    for word in (0, field, documented, S.REDO_SWEPT_SUBSTEP0 << 3 | S.REDO_PRIMAL | S.REDO_DROPPED, 0x7fffffff & ~field):
        assert swept_substeps(word) == (word & field) >> 8
    assert swept_substeps(field) == (1 << S.REDO_SWEPT_SUBSTEPS) - 1 and S.REDO_SWEPT_SUBSTEP0 == 1 << 8


def test_handon_why_word_fields(words):
    K, S = words.K, _public()
    old = 0x2a0d1103
    for reason in (S.WHY_CONTACTS, S.WHY_ROWS, S.WHY_DENSE_SLOTS, S.WHY_ROW_STORAGE, S.WHY_CANDIDATES, S.WHY_SOLVER, 0x3f):
        status = (reason << K["WHY_SHIFT"]) | K["ST_HANDON"]
        field = lambda w, sh: (w >> sh) & S.WHY_FIELD
        w = words.handon_why_word(1, old, status, 9)  # the fast tier: its own field and the substep; the general tier's stays, the large tier's is cleared
        assert (field(w, S.WHY_FAST_SHIFT), field(w, S.WHY_GENERAL_SHIFT), field(w, S.WHY_SUBSTEP_SHIFT), field(w, S.WHY_LARGE_SHIFT)) == (reason, field(old, S.WHY_GENERAL_SHIFT), 9, 0)
        w = words.handon_why_word(2, old, status, 9)
        assert (field(w, S.WHY_FAST_SHIFT), field(w, S.WHY_GENERAL_SHIFT), field(w, S.WHY_SUBSTEP_SHIFT), field(w, S.WHY_LARGE_SHIFT)) == (field(old, S.WHY_FAST_SHIFT), reason, 9, 0)
        w = words.handon_why_word(3, old, status, 9)  # the large tier adds its field to the word
        assert w == old | (reason << S.WHY_LARGE_SHIFT)


def _plans(words):
    for cls, knobs in PLANS:
        yield plan_key(cls, knobs), words.plan(cls, knobs)


def _probe_peaks(W):
    """peaks around every threshold, all together and one at a time, on a coarser lattice too"""
    th = thresholds(W)
    vals = {name: sorted({0} | {max(v + d, 0) for v in th[name] for d in (-1, 0, 1)}) for name in PEAKS[:4]}
    out = peak_cases(W)
    for n, c, t, y in itertools.product(vals["nefc"][::2], vals["ncon"][::3], vals["ntwo"][::3], vals["y"][::2]):
        out.append([n, c, t, y, 0])
    return out


def test_a_tier_does_not_send_back_up_what_the_tier_above_sent_down(words):
    for key, W in _plans(words):
        for lt in (2, 3, 4):
            for pk in _probe_peaks(W):
                if words.next_tier(2, pk, lt, 0) == 1:
                    assert words.next_tier(1, pk, lt, 0) == 1, (key, lt, pk)
                if words.next_tier(3, pk, lt, 0) == 2:
                    assert words.next_tier(2, pk, lt, 0) == 2, (key, lt, pk)
                if words.next_tier(3, pk, lt, 0) == 1:
                    assert words.next_tier(1, pk, lt, 0) == 1, (key, lt, pk)


def test_policy_is_monotone(words):
    for key, W in _plans(words):
        base = peak_cases(W)
        for lt, rows in ((W["last_tier"], 0), (4, T4_ROWS)):
            for tier in (1, 2, 3, 4):
                for pk in base:
                    t0 = words.next_tier(tier, pk, lt, rows)
                    for k in range(5):
                        for d in (1, 7, 1000):
                            up = list(pk)
                            up[k] += d
                            assert words.next_tier(tier, up, lt, rows) >= t0, (key, tier, lt, rows, pk, up)
        for pk in base:
            for v0, v1 in ((0.0, 30.5), (30.5, 61.0)):
                assert words.launch_cost(pk, v1) >= words.launch_cost(pk, v0)
            c0 = words.launch_cost(pk, 0.0)
            for k in range(5):
                for d in (1, 7, 1000):
                    up = list(pk)
                    up[k] += d
                    assert words.launch_cost(up, 0.0) >= c0, (key, pk, up)
    # a costlier env is never launched later
    buckets = [words.order_bucket(1, 0, 0, 0, c) for c in range(0, 130)]
    assert all(a >= b for a, b in zip(buckets, buckets[1:])) and buckets[0] == words.K["ORDER_BUCKETS"] - 1 and buckets[-1] == 1
    assert all(1 <= b < words.K["ORDER_BUCKETS"] for b in buckets)  # (bucket 0 is the fresh envs', the last one the envs of other launches)


def test_a_fresh_env_heads_the_launch_and_never_starts_in_tier_4(words):
    K = words.K
    for cost in (0, 23, 24, 62, 64, 1000):
        for masked in (0, 1):
            assert words.order_bucket(1, masked, 1, 1, cost) == 0
        assert words.order_bucket(1, 1, 0, 1, cost) == K["ORDER_BUCKETS"]  # (not in this step: not this launch's)
        for tier in (2, 3, 4):
            for fresh in (0, 1):
                assert words.order_bucket(tier, 0, 0, fresh, cost) == K["ORDER_BUCKETS"]
    for launch4 in (0, 1):
        for tier in (1, 2, 3, 4):
            assert words.start_tier(tier, 1, launch4) == (2 if tier == 4 else tier) != 4
        assert [words.start_tier(t, 0, launch4) for t in (1, 2, 3, 4)] == [1, 2, 3, 4 if launch4 else 3]


def test_chunk_record_merge_is_commutative_and_idempotent(words):
    K = words.K
    peak_words = [K[n] for n in ("REC_PK_NEFC", "REC_PK_NCON", "REC_PK_NTWO", "REC_PK_Y", "REC_PK_ACT")]
    assert peak_words == [0, 1, 2, 3, 4] and K["REC_STATUS"] < K["CHUNK_REC"]

    def record(pk, status):  # a record as a chunk stores it: the peaks, the newest pass's counts (not merged), the status
        r = [0] * K["CHUNK_REC"]
        for w, v in zip(peak_words, pk):
            r[w] = v
        r[K["REC_NCON"]], r[K["REC_NEFC"]], r[K["REC_ITERS"]], r[K["REC_STATUS"]] = 3, 17, 2, status
        return r

    sides = [([40, 9, 3, 700, 12], K["ST_DROPPED"]), ([41, 2, 7, 10, 30], 0), ([0, 0, 0, 0, 0], 0), ([5, 16, 0, 701, 1], K["ST_DROPPED"])]
    for (pa, sa), (pb, sb) in itertools.product(sides, sides):
        ab = words.chunk_rec_merge(pa, sa, record(pb, sb))
        assert ab == words.chunk_rec_merge(pb, sb, record(pa, sa))
        assert ab == ([max(x, y) for x, y in zip(pa, pb)], sa | sb)
        assert words.chunk_rec_merge(ab[0], ab[1], record(pb, sb)) == ab  # merging the same record again changes nothing
    assert words.chunk_rec_merge(pa, sa, record(pa, sa)) == (pa, sa)


# ---------------------------------------------------------------------------------------------------------------- c. the public names
def test_python_names_equal_the_header(words):
    S = _public()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uhc_amd.h")).read(), flags=re.S)
    defs = {}
    for name, val in re.findall(r"#define (UHC_(?:REDO|HANDON)_[A-Z0-9_]+) +(\(1 << \d+\)|0x[0-9a-fA-F]+|\d+)\s", src):
        m = re.match(r"\(1 << (\d+)\)", val)
        defs[name] = 1 << int(m.group(1)) if m else int(val, 0)
    mine = {("UHC_" + k if k.startswith("REDO_") else "UHC_HANDON_" + k[4:]): v for k, v in vars(S).items() if k.startswith(("REDO_", "WHY_")) and isinstance(v, int)}
    assert len(defs) == 23 and mine == defs
    assert "UHC_ABI_VERSION 11" in src  # naming the bits changed none of them


def test_python_debug_bits_and_trace_words_equal_the_header():
    """enum UhcDebug, enum UhcTraceWord, UHC_DEBUG_EXP_MASK, UHC_PROF_WORDS and UHC_TRACE_CONSUMER_WORDS of include/uhc_amd.h against uhc_amd/_capi.py's DEBUG_* / TRACE_* /
    PROF_WORDS, and uhc_amd/sim.py's re-exports"""
    from uhc_amd import _capi
    S = _public()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uhc_amd.h")).read(), flags=re.S)
    defs = {}
    for enum in ("UhcDebug", "UhcTraceWord"):
        body = re.search(r"enum %s \{(.*?)\};" % enum, src, flags=re.S).group(1)
        entries = [e.strip() for e in body.split(",") if e.strip()]
        for e in entries:
            name, val = re.fullmatch(r"(UHC_[A-Z0-9_]+) = (1 << \d+|\d+)", e).groups()
            defs[name] = 1 << int(val[5:]) if val.startswith("1 << ") else int(val)
    for name in ("UHC_PROF_WORDS", "UHC_TRACE_CONSUMER_WORDS"):
        defs[name] = int(re.search(r"#define %s (\d+)\s" % name, src).group(1))
    mask = re.search(r"#define UHC_DEBUG_EXP_MASK \((.*?)\)\n", src).group(1).split(" | ")
    defs["UHC_DEBUG_EXP_MASK"] = sum(defs[n] for n in mask)
    assert len(mask) == len(set(mask)) == 5 and defs["UHC_DEBUG_EXP_MASK"] == 0x1f00
    assert [defs[n] for n in defs if n.startswith("UHC_DEBUG_") and n != "UHC_DEBUG_EXP_MASK"] == [1 << k for k in range(13)]  # thirteen bits, in order
    for mod in (_capi, S):
        mine = {"UHC_" + k: v for k, v in vars(mod).items() if k.startswith(("DEBUG_", "TRACE_", "PROF_WORDS")) and isinstance(v, int)}
        assert len(defs) == 13 + 9 + 3 and mine == defs, (mod.__name__, set(mine.items()) ^ set(defs.items()))
    # today's numbers: the record's length, the trace's words
    assert (defs["UHC_PROF_WORDS"], defs["UHC_TRACE_TAKEN"], defs["UHC_TRACE_LET_GO"], defs["UHC_TRACE_HANDON_SUBSTEP"], defs["UHC_TRACE_CONSUMER"], defs["UHC_TRACE_GATE"], defs["UHC_TRACE_TAKEN4"],
            defs["UHC_TRACE_LET_GO4"], defs["UHC_TRACE_HANDON_SUBSTEP3"], defs["UHC_TRACE_CHUNK_WAIT"]) == (40, 0, 1, 6, 8, 16, 21, 22, 23, 24)
    assert "UHC_ABI_VERSION 11" in src  # naming the bits changed none of them
