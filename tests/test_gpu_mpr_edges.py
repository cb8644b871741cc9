"""The convex narrow phase on the device, on every serving path, against the CPU oracle -- on the case table of tests/mpr_cases.py, which tests/test_mpr_cases_cpu.py
holds against plain geometry.

PATHS.  chain: the tier chain, UHC_FORCE_GENERAL=0 -- two bodies fit the dense fast tier, which serves MPR with mpr_wave.  general: UHC_FORCE_GENERAL=1, the general tier's
one-wave kernel, mpr_wave again.  sticky: set_kernel_path(2) with UHC_TIER_MARKS "-1,..." (up to the general tier above -1 rows, never down), where the general tier's
envs are computed by its two-wave queue consumers (uhc_k_general_q.hip: mpr_wave_mw, the requests of a round dealt out over two waves through an LDS mailbox).  The
sticky launch serves CONTROL STEPS only (set_state's forward pass takes the plain chain), and the consumers are sized from queue counts the host sees with a lag: the
first step is the fast tier's (the env moves up), the second finds the queue filled but no consumers sized yet (the chained general launch computes it), the third is
the consumers'.  Every step starts from the case's own state, and the third is compared with the oracle after the same one step; the tier trace's consumer record says
how many envs the consumers computed.

SWITCHES (UHC_DEBUG).  unset: every model of the table is staged by the fast, general and large tier (tests/test_mpr_cases_cpu.py asks the plan) -- hull vertices in LDS.
DEBUG_NO_VSTAGE: vertices from global memory (mpr_wave_mw<false> in the consumers).  DEBUG_NO_BOX_CULL: every pair past the bounding spheres is a candidate.

BARS.  Against the oracle: ncon and nefc equal, qacc within atol 1e-8 / rtol 1e-9 (test_exact_solver_forward's bar for two exact solves), nothing failed, dropped or
swept.  A case the oracle itself answers discontinuously (its qacc moves by more than 1e-8 under a 1e-15 turn: at most 2 % of the table, asserted on the CPU) is judged
by tests/test_gpu_parity_200.py's rule: the device lies on one of the oracle's own branches to 1e-7, or no further from the oracle than twice the oracle's spread.
Within one path the switches change where bytes are read from and which pairs are looked at, never the arithmetic: ncon, nefc and qacc are bit for bit equal."""
import contextlib
import os

import numpy as np
import pytest

from tests import mpr_cases as M
from tests.helpers import passive_ctrl

pytestmark = pytest.mark.gpu

PATHS = ("chain", "general", "sticky")
ATOL, RTOL = 1e-8, 1e-9
MARKS = "-1,-1,-1,-1,-1,-1,8,7"


def _switches():
    from uhc_amd import sim as S
    return {"unset": 0, "no_vstage": S.DEBUG_NO_VSTAGE, "no_box_cull": S.DEBUG_NO_BOX_CULL}


@contextlib.contextmanager
def _environ(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _device(m, q, v, path, dbg):
    """The envs (q, v) of model m on `path` under the debug bits `dbg` -> the observables as numpy arrays, `consumed`: env-steps the general tier's consumers computed"""
    import torch
    from uhc_amd import sim as S
    n = len(q)
    ctrl = passive_ctrl(m)
    sticky = path == "sticky"
    word = dbg | (S.DEBUG_TRACE if sticky else 0)
    with _environ(UHC_FORCE_GENERAL="1" if path == "general" else "0", UHC_DEBUG=word if word else None, UHC_TIER_MARKS=MARKS if sticky else None):
        b = S.SimBatch(m, ctrl, n)
    tq, tv = torch.from_numpy(np.ascontiguousarray(q)), torch.from_numpy(np.ascontiguousarray(v))
    consumed = 0
    if sticky:
        b.set_kernel_path(2)
        act = torch.zeros(n, ctrl.action_dim, dtype=torch.float64, device="cuda")
        for k in range(3):
            b.set_state(tq, tv)
            b.field(S.F_STAGE_PROF).zero_()
            b.simulate(act, act)
            b.sync()
        consumed = int(b.field(S.F_STAGE_PROF)[:, S.TRACE_CONSUMER + 3].sum().item())
    else:
        b.set_state(tq, tv)
        b.sync()
    out = {k: b.field(getattr(S, f)).cpu().numpy().copy() for k, f in
           dict(ncon="F_NCON", nefc="F_NEFC", qacc="F_QACC", redo="F_REDO", overflow="F_EFC_OVERFLOW", fail="F_FAIL", why="F_HANDON_WHY", tier="F_TIER").items()}
    out["consumed"] = consumed
    b.close()
    return out


def _where_computed(dev, path, n):
    """assert that the envs were computed where the path claims -> the tier's name for the report"""
    from uhc_amd.sim import REDO_GENERAL, REDO_LARGE
    if path == "chain":
        assert (dev["redo"] == 0).all(), [hex(int(w)) for w in dev["redo"]]  # the fast tier kept every env: nothing redone, nothing handed on
        return "fast"
    assert not (dev["redo"] & REDO_LARGE).any(), [hex(int(w)) for w in dev["redo"]]
    if path == "sticky":
        assert (dev["redo"] & REDO_GENERAL).all() and (dev["tier"] == 2).all(), ([hex(int(w)) for w in dev["redo"]], dev["tier"].tolist())
        assert dev["consumed"] == n, (dev["consumed"], n)  # every env of the third step went through a two-wave consumer
        return "general, two-wave consumers"
    return "general"


def _against_oracle(label, dev, ref, spread=None, twins=None, envs=None):
    """Every env against the oracle's answer -> (worst |dqacc| of the cases held to the bar, cases judged by the oracle's branches).  Figures are printed before they are asserted."""
    from uhc_amd.sim import REDO_DROPPED, REDO_SWEPT
    envs = list(range(len(ref))) if envs is None else envs
    worst, aside, bad = 0.0, [], []
    for k, e in enumerate(envs):
        r = ref[e]
        same = dev["ncon"][k] == r["ncon"] and dev["nefc"][k] == r["nefc"]
        err = float(np.abs(dev["qacc"][k] - r["qacc"]).max()) if same else np.inf
        ok = same and bool((np.abs(dev["qacc"][k] - r["qacc"]) <= ATOL + RTOL * np.abs(r["qacc"])).all())
        if spread is not None and spread[e] > M.SPREAD_BAR:
            # a discontinuity of the contact model: on one of the oracle's own branches, or inside their spread
            near = min([err] + [float(np.abs(dev["qacc"][k] - t[e]["qacc"]).max()) for t in twins if t[e]["ncon"] == dev["ncon"][k] and t[e]["nefc"] == dev["nefc"][k]])
            aside.append((e, err, near, float(spread[e])))
            if not (near <= 1e-7 or err <= 2.0 * spread[e]):
                bad.append((e, "off every branch of the oracle", err, near, float(spread[e])))
            continue
        worst = max(worst, err)
        if not ok:
            bad.append((e, int(dev["ncon"][k]), r["ncon"], int(dev["nefc"][k]), r["nefc"], err))
    print(f"MPR EDGES {label}: {len(envs)} cases, worst |dqacc| {worst:.2e}, judged by the oracle's branches {[(e, f'{a:.1e}', f'{b:.1e}') for e, a, b, _ in aside]}")
    assert not bad, (label, bad[:8])
    assert not dev["fail"].any() and not dev["overflow"].any(), label
    assert not (dev["redo"] & (REDO_DROPPED | REDO_SWEPT)).any(), (label, [hex(int(w)) for w in dev["redo"]])
    return worst, len(aside)


def _bitwise(label, a, b):
    import torch
    for k in ("ncon", "nefc", "qacc"):
        assert torch.equal(torch.from_numpy(a[k]), torch.from_numpy(b[k])), (label, k, float(np.abs(a[k].astype(np.float64) - b[k]).max()))


# ------------------------------------------------------------------ two bodies: every hull family, every path, every switch
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(M.FAMILIES))
def test_family_matches_oracle_on_every_path(name, path):
    m = M.family_model(name)
    q, v, tags = M.family_cases(name)
    stepped = path == "sticky"
    ref = M.family_reference(name, stepped)
    spread, twins = M.family_spread(name, stepped)
    hits = sum(r["ncon"] for r in ref)
    assert hits >= 10 and len(ref) - hits >= 10  # the sample has touching and separated pairs (the CPU file asserts the same of the forward pass)
    for envs in M.batches():
        runs = {}
        for sw, dbg in _switches().items():
            dev = runs[sw] = _device(m, q[envs], v[envs], path, dbg)
            where = _where_computed(dev, path, len(envs))
            staged = "global" if sw == "no_vstage" else "LDS"
            _against_oracle(f"{name:16s} {path:8s} {sw:12s} [{where}, vertices from {staged}] envs {envs[0]}-{envs[-1]}", dev, ref, spread, twins, envs)
        _bitwise((name, path, "staging on / off"), runs["unset"], runs["no_vstage"])
        _bitwise((name, path, "box cull on / off"), runs["unset"], runs["no_box_cull"])


# ------------------------------------------------------------------ more than one pair per round
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["three", "four"])
def test_three_and_four_bodies_match_oracle(name, path):
    """3 pairs: an odd number of requests in a round, the last served singly; 6 pairs: served two by two.  Hulls of 4, 8, 50 (and 64) vertices in one env; 16 envs from every
    pair overlapping to most apart, so the rounds run with every request count from the pairs' number down."""
    m, q, v = M.multi_scene(name)
    ref = M.multi_reference(name, path == "sticky")
    runs = {}
    for sw, dbg in _switches().items():
        dev = runs[sw] = _device(m, q, v, path, dbg)
        where = _where_computed(dev, path, len(q))
        _against_oracle(f"{name:16s} {path:8s} {sw:12s} [{where}]", dev, ref)
    _bitwise((name, path, "staging on / off"), runs["unset"], runs["no_vstage"])
    _bitwise((name, path, "box cull on / off"), runs["unset"], runs["no_box_cull"])


@pytest.mark.parametrize("path", PATHS)
def test_66_candidates_take_a_second_trip(path):
    """12 rods: with the box cull off all 66 pairs are candidates -- a second trip of the c0 loop with a 2-pair tail; with it on, a few.  Both equal each other bit for bit,
    and the oracle (which culls by bounding spheres alone)."""
    m, q, v = M.multi_scene("rods12")
    ref = M.multi_reference("rods12", path == "sticky")
    runs = {}
    for sw, dbg in _switches().items():
        dev = runs[sw] = _device(m, q, v, path, dbg)
        if path == "sticky":
            assert dev["consumed"] == len(q) and (dev["tier"] == 2).all()
        _against_oracle(f"rods12           {path:8s} {sw:12s}", dev, ref)
    _bitwise(("rods12", path, "staging on / off"), runs["unset"], runs["no_vstage"])
    _bitwise(("rods12", path, "box cull on / off"), runs["unset"], runs["no_box_cull"])


@pytest.mark.parametrize("path", PATHS)
def test_253_candidates_fit_the_candidate_list(path):
    """23 rods on slide joints, the box cull off: 253 candidates, four trips, no flag; equal to the run with the cull on and to the oracle."""
    from uhc_amd import sim as S
    m, q, v = M.multi_scene("rods23")
    ref = M.multi_reference("rods23", path == "sticky")
    on = _device(m, q, v, path, 0)
    off = _device(m, q, v, path, S.DEBUG_NO_BOX_CULL)
    for sw, dev in (("unset", on), ("no_box_cull", off)):
        _against_oracle(f"rods23           {path:8s} {sw:12s}", dev, ref)
        assert not any((int(w) >> s) & S.WHY_CANDIDATES for w in dev["why"] for s in (S.WHY_FAST_SHIFT, S.WHY_GENERAL_SHIFT, S.WHY_LARGE_SHIFT)), [hex(int(w)) for w in dev["why"]]
    _bitwise(("rods23", path, "box cull on / off"), on, off)


@pytest.mark.parametrize("path", PATHS)
def test_batch_independence(path):
    """A hit, a miss, a tie (an exact quarter turn, face on face) and the small box deep inside the large one in neighbouring envs of one batch equal the same cases run
    alone, bit for bit."""
    m = M.family_model("box")
    q, v, tags = M.family_cases("box")
    ref = M.family_reference("box")
    pick = [next(e for e, t in enumerate(tags) if t == "random" and ref[e]["ncon"] == 1), next(e for e, t in enumerate(tags) if t == "random" and ref[e]["ncon"] == 0),
            next(e for e, t in enumerate(tags) if t == "quarter" and ref[e]["ncon"] == 1), next(e for e, t in enumerate(tags) if t == "inside")]
    assert ref[pick[3]]["ncon"] == 1
    mixed = _device(m, q[pick], v[pick], path, 0)
    for k, e in enumerate(pick):
        alone = _device(m, q[[e]], v[[e]], path, 0)
        _bitwise(("box", path, f"case {e} ({tags[e]}) in the mixed batch and alone"), {f: mixed[f][k:k + 1] for f in ("ncon", "nefc", "qacc")}, alone)


@pytest.mark.parametrize("path", PATHS)
def test_first_maximum_wins_across_the_trips_of_a_large_hull(path):
    """The drum scene (tests/mpr_cases.py): an 80-vertex hull whose 40 bottom vertices tie exactly in the first support query, in both trips of the scan.  Which of them is
    returned decides where on the face the contact lands -- the oracle's qacc moves by 4 to 36 when another comes first (tests/test_mpr_cases_cpu.py) -- so these cases
    are discontinuities by the 1e-15 rule; they are NOT set aside here.  The tie is exact in both arithmetics (identity and z-turn matrices, one z for the whole face: no
    product is rounded, contracted or not) and every other query is in general position, so the device has to take the oracle's own branch: the first maximum, to the
    bar of every other case."""
    from uhc_amd import sim as S
    m, q, v = M.drum_scene()
    ref = M.drum_reference(path == "sticky")
    runs = {}
    for sw, dbg in (("unset", 0), ("no_vstage", S.DEBUG_NO_VSTAGE)):
        dev = runs[sw] = _device(m, q, v, path, dbg)
        if path == "sticky":
            assert dev["consumed"] == len(q) and (dev["tier"] == 2).all()
        _against_oracle(f"drum             {path:8s} {sw:12s}", dev, ref)
    _bitwise(("drum", path, "staging on / off"), runs["unset"], runs["no_vstage"])


# ------------------------------------------------------------------ the capacity edge: more candidates than the list holds
@pytest.mark.parametrize("path", PATHS)
def test_276_candidates_are_flagged_and_the_cull_brings_them_back(path):
    """24 rods on slide joints: 276 pairs past the bounding spheres.  With the box cull on a few are candidates and the env equals the oracle with no flag.  With it off the
    candidates beyond CAND_CAP = 256 are not looked at, in any tier (cand[rank] is stored under rank < CAND_CAP; rowMisc holds 256 ints in every tier:
    tests/test_mpr_cases_cpu.py): every tier that has a next one hands the env on with UHC_WHY_CANDIDATES in its field of UHC_F_HANDON_WHY, the last one drops the pairs and
    says so -- UHC_REDO_DROPPED in UHC_F_REDO, UHC_F_EFC_OVERFLOW until the next set_state -- and the step stays finite and unfailed."""
    from uhc_amd import sim as S
    m, q, v = M.multi_scene("rods24")
    ref = M.multi_reference("rods24", path == "sticky")
    on = _device(m, q, v, path, 0)
    _against_oracle(f"rods24           {path:8s} unset       ", on, ref)
    assert (on["why"] == 0).all() or not any((int(w) >> s) & S.WHY_CANDIDATES for w in on["why"] for s in (S.WHY_FAST_SHIFT, S.WHY_GENERAL_SHIFT, S.WHY_LARGE_SHIFT))
    off = _device(m, q, v, path, S.DEBUG_NO_BOX_CULL)
    print(f"MPR EDGES rods24 {path} no_box_cull: redo {[hex(int(w)) for w in off['redo']]} why {[hex(int(w)) for w in off['why']]} overflow {off['overflow'].tolist()} ncon {off['ncon'].tolist()}")
    assert (off["redo"] & S.REDO_DROPPED).all() and (off["overflow"] > 0).all() and not off["fail"].any()
    first = S.WHY_FAST_SHIFT if path == "chain" else S.WHY_GENERAL_SHIFT  # the first tier that computed the env (sticky: the general tier's consumer, by the third step)
    assert all((int(w) >> first) & S.WHY_CANDIDATES for w in off["why"]), [hex(int(w)) for w in off["why"]]
    assert np.isfinite(off["qacc"]).all()
