"""CPU: the window rule of a sliding live stream (uhc_amd/csrc/uhc_live_window.h: uhc_lw_discard), compiled for the host (tests/live_window_probe.cpp) --
the function uhc_live.hip's slide kernel calls.  Over every small case: S stays inside the window and behind the consumer, every read of the env kernels
resolves to the same global frame after the slide as before it, and a slice that is not full never slides.  Then whole sessions on a host model
(tests/live_window_cases.py), the model's rule being the header's: no read ever maps to a discarded frame."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import probe_build
from tests import live_window_cases as LW



def build_probe():
    """tests/live_window_probe.cpp + uhc_live_window.h -> uhc_amd/csrc/build/live_window_probe.so with the host compiler: no hipcc, no HIP header."""
    return probe_build.build_probe("live_window_probe.so", ["tests/live_window_probe.cpp"], ["uhc_amd/csrc/uhc_live_window.h"])


@pytest.fixture(scope="module")
def probe():
    return C.CDLL(build_probe())


def _discard(P, cases):
    a = np.ascontiguousarray(cases, dtype=np.int32).reshape(-1, 4)
    out = np.full(len(a), -99, dtype=np.int32)
    P.uhc_live_window_probe_discard(C.c_int(len(a)), a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


@pytest.fixture(scope="module")
def grid(probe):
    """every (len, cap, start_ind, cur_t) with cap <= 8, len <= cap, -8 <= start_ind <= 8, 0 <= cur_t <= 16, start_ind + cur_t >= 0 -- and the rule's S"""
    cases = np.array([(ln, cap, si, t) for cap in range(1, 9) for ln in range(0, cap + 1) for si in range(-8, 9) for t in range(0, 17) if si + t >= 0], dtype=np.int32)
    assert len(cases) > 10000
    return cases, _discard(probe, cases)


def test_s_stays_inside_the_window_and_behind_the_consumer(grid):
    cases, S = grid
    ln, cap, si, t = cases.T
    assert (S >= 0).all()
    assert (S <= np.maximum(ln - 1, 0)).all()
    assert (S <= si + t).all()
    full = ln == cap
    assert np.array_equal(S[full], np.minimum(si + t, ln - 1)[full])  # the rule itself, where the slice is full
    assert S.max() == 7 and (S[full] == 0).any()                      # (both ends occur in the grid)


def test_a_slice_that_is_not_full_never_slides(grid):
    cases, S = grid
    ln, cap = cases[:, 0], cases[:, 1]
    assert (ln < cap).any() and not S[ln < cap].any()


def test_every_read_resolves_to_the_same_global_frame_after_the_slide(grid):
    cases, S = grid
    ln, cap, si, t = (cases[:, k].astype(np.int64) for k in range(4))
    keep = ln >= 1
    for ahead in range(5):  # t = cur_t .. cur_t + 4
        before = np.minimum(si + t + ahead, ln - 1)
        after = np.minimum(si - S + t + ahead, ln - S - 1) + S
        assert np.array_equal(before[keep], after[keep]), ahead
        assert (before[keep] >= 0).all() and ((after - S)[keep] >= 0).all()  # ... and both stay inside their slices


def test_the_python_model_restates_the_rule(grid):
    cases, S = grid
    assert [LW.discard(*map(int, c)) for c in cases] == S.tolist()
    # memory that does not hold the invariant, and sums beyond 32 bits: S stays in 0 .. len - 1
    odd = [(4, 4, -9, 3), (4, 4, 2**31 - 1, 2**31 - 1), (4, 4, -2**31, -2**31), (0, 0, 5, 5), (1, 1, 7, 7), (-3, -3, 1, 1), (5, 4, 3, 3)]
    assert _discard(C.CDLL(build_probe()), odd).tolist() == [0, 3, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("cap", [4, 5, 8])
def test_a_session_never_reads_a_discarded_frame(probe, cap):
    rule = lambda *a: int(_discard(probe, [a])[0])  # noqa: E731  (the header's function drives the model)
    w = LW.session(cap, head=3, steps=40, ahead=4, rule=rule)
    assert w.base == 43 - w.len and w.len <= cap and w.moved > 0
    if cap == 4:
        assert w.moved == 3 * 39  # every push after the first slides by one and moves three records
    # the same session without sliding runs out of room at `cap`
    with pytest.raises(AssertionError):
        LW.session(cap, head=3, steps=40, ahead=4, slide=False)


def test_the_move_is_correct_lane_by_lane_when_the_ranges_overlap(probe):
    """The kernel's copy order, serialised by lane (tests/live_window_probe.cpp): records S .. len - 1 to slots 0 .., overlapping when S < len - S."""
    width, lanes = 11, 4
    for cap, si, t in itertools.product((2, 3, 8), (-2, 0, 1), (0, 1, 2, 3, 9)):
        if si + t < 0:
            continue
        sl = np.repeat(np.arange(cap, dtype=np.float64), width).reshape(cap, width) * 10 + np.arange(width)
        want = sl.copy()
        st = np.array([cap, si, 0, 0], dtype=np.int32)
        S = probe.uhc_live_window_probe_slide(cap, width, lanes, sl.ctypes.data_as(C.c_void_p), t, st.ctypes.data_as(C.c_void_p))
        assert S == LW.discard(cap, cap, si, t)
        if S:
            assert np.array_equal(sl[:cap - S], want[S:]) and st.tolist() == [cap - S, si - S, S, cap - S]
        else:
            assert np.array_equal(sl, want) and st.tolist() == [cap, si, 0, 0]
