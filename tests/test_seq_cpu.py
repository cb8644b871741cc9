"""CPU: uhc_amd/csrc/uhc_seq.h -- the sequence rules the post-processing kernels share (row-count clamp, first row or skip, model clamp, clip lookup, packed bytes,
the ordered mean) -- compiled for the host (tests/seq_probe.cpp) and run at the edges at which each can go wrong.  What the header promises is that no index,
whatever it holds, leaves the arrays: every result here is checked to lie in its range, not only to be the expected one."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import probe_build

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
QNAN_BITS = 0x7ff8000000000000


def build_probe():
    """tests/seq_probe.cpp + uhc_seq.h -> uhc_amd/csrc/build/seq_probe.so with the host compiler: no hipcc, no HIP header."""
    return probe_build.build_probe("seq_probe.so", ["tests/seq_probe.cpp"], ["uhc_amd/csrc/uhc_seq.h"], probe_build.NO_CONTRACT)


@pytest.fixture(scope="module")
def P():
    L = C.CDLL(build_probe())
    L.uhc_seq_probe_rows.argtypes = [C.c_int, C.c_int]
    L.uhc_seq_probe_start.argtypes, L.uhc_seq_probe_start.restype = [C.c_longlong, C.c_int, C.c_longlong], C.c_longlong
    L.uhc_seq_probe_model.argtypes = [C.c_void_p, C.c_longlong, C.c_int]
    L.uhc_seq_probe_clip.argtypes = [C.c_void_p, C.c_int, C.c_longlong]
    L.uhc_seq_probe_packed_byte.argtypes = [C.c_void_p, C.c_int]
    L.uhc_seq_probe_nan.restype = C.c_double
    L.uhc_seq_probe_mean.argtypes, L.uhc_seq_probe_mean.restype = [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int], C.c_double
    return L


def _ptr(x):
    return x.ctypes.data_as(C.c_void_p)


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_nan_is_the_quiet_nan_numpy_writes_for_an_empty_mean(P):
    assert _bits(P.uhc_seq_probe_nan()) == QNAN_BITS


@pytest.mark.parametrize("cap", [1, 7, INT_MAX])
def test_rows_are_clamped_to_0_cap(P, cap):
    for r, want in [(INT_MIN, 0), (-1, 0), (0, 0), (cap, cap), (INT_MAX, cap)] + ([(cap + 1, cap)] if cap < INT_MAX else []) + ([(cap - 1, cap - 1)] if cap > 1 else []):
        assert P.uhc_seq_probe_rows(r, cap) == want, (r, cap)


@pytest.mark.parametrize("n,T", [(10, 3), (10, 10), (3, 1), (2 ** 31, 5)])
def test_start_is_the_first_row_or_skip(P, n, T):
    for g, want in [(-1, -1), (0, 0), (n - T, n - T), (n - T + 1, -1), (-2 ** 63, -1), (2 ** 63 - 1, -1)]:
        assert P.uhc_seq_probe_start(g, T, n) == want, (g, T, n)


def test_start_of_an_empty_sequence_and_of_no_rows(P):
    n = 10
    assert P.uhc_seq_probe_start(n, 0, n) == n  # T = 0 reads nothing: the row behind the last one is a start like any other ...
    assert P.uhc_seq_probe_start(n + 1, 0, n) == -1  # ... one further is not
    assert P.uhc_seq_probe_start(0, 0, 0) == 0 and P.uhc_seq_probe_start(0, 1, 0) == -1 and P.uhc_seq_probe_start(-1, 0, 0) == -1 and P.uhc_seq_probe_start(1, 0, 0) == -1


@pytest.mark.parametrize("n", [1, 2, 5])
def test_model_outside_the_range_reads_as_0(P, n):
    assert P.uhc_seq_probe_model(None, 3, n) == 0  # no table: model 0 for every entry
    table = np.array([-1, 0, n - 1, n, INT_MIN, INT_MAX], dtype=np.int32)
    for s, want in enumerate([0, 0, n - 1, 0, 0, 0]):
        assert P.uhc_seq_probe_model(_ptr(table), s, n) == want, (s, n)


def _clip(P, start, f):
    start = np.ascontiguousarray(start, dtype=np.int32)
    c = P.uhc_seq_probe_clip(_ptr(start), len(start), int(f))
    assert 0 <= c < len(start), (start, f, c)  # whatever the table holds
    return c


def test_clip_of_one_clip(P):
    for f in (-5, 0, 1, 10 ** 12):
        assert _clip(P, [0], f) == 0 and _clip(P, [7], f) == 0


@pytest.mark.parametrize("start,n_frames", [([0, 4, 9], 12), ([0, 1, 2, 3], 4), ([3, 8], 20), ([0, 5, 5, 9], 11), (list(range(0, 70, 7)), 75)])
def test_clip_of_is_the_last_clip_whose_start_is_at_most_f(P, start, n_frames):
    s = np.array(start)
    for f in sorted({s[0] - 1, n_frames - 1, n_frames, 2 ** 40} | set(s) | set(s - 1)):
        want = int(np.clip(np.searchsorted(s, f, "right") - 1, 0, len(s) - 1))
        assert _clip(P, start, int(f)) == want, (start, f)
    for f in range(-2, n_frames + 2):  # every frame, and a few outside the bank
        assert _clip(P, start, f) == int(np.clip(np.searchsorted(s, f, "right") - 1, 0, len(s) - 1)), (start, f)
    assert _clip(P, start, s[0] - 1) == 0  # below the first start: clip 0
    for c, v in enumerate(start):
        if start.count(v) == 1:
            assert _clip(P, start, v) == c and (c == 0 or _clip(P, start, v - 1) == c - 1)


@pytest.mark.parametrize("start", [[9, 4, 0], [0, 8, 3, 12, 1], [-5, -1, 2], [-1, -1, -1], [INT_MAX, INT_MIN, 0, INT_MAX], [5, 5, 5, 5, 5, 5, 5]])
def test_clip_of_stays_inside_the_table_whatever_it_holds(P, start):
    for f in [-2 ** 40, INT_MIN, -6, -1, 0, 1, 3, 4, 5, 8, 9, 12, INT_MAX, 2 ** 40] + start:
        _clip(P, start, f)  # (asserts the range)


def test_packed_byte_reads_all_24_positions(P):
    rng = np.random.default_rng(5)
    for _ in range(4):
        to_model = np.concatenate(([0], 1 + rng.permutation(23)))  # h_smpl_to_model: a permutation that keeps the root at 0
        w = [0, 0, 0]
        for m, j in enumerate(to_model):  # uhc_smpl.hip's pack_slot_table: the slot of SMPL joint j is m
            w[j >> 3] |= int(m) << (8 * (j & 7))
        words = np.array(w, dtype=np.uint64)
        for m, j in enumerate(to_model):
            assert P.uhc_seq_probe_packed_byte(_ptr(words), int(j)) == m
    words = np.array([0xfffefdfcfbfaf9f8, 0, 0x8000000000000000], dtype=np.uint64)  # bytes above 127 come out unsigned
    assert [P.uhc_seq_probe_packed_byte(_ptr(words), i) for i in (0, 7, 8, 23)] == [0xf8, 0xff, 0, 0x80]


def _mean(P, rows, stride, k, g0, n):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    return P.uhc_seq_probe_mean(_ptr(rows), stride, k, g0, n)


def test_mean_over_no_row_is_nan_and_over_one_row_is_the_row(P):
    rows = np.arange(12.0).reshape(3, 4)
    for n in (0, -1, INT_MIN):
        assert _bits(_mean(P, rows, 4, 1, 0, n)) == QNAN_BITS
    for g0 in range(3):
        for k in range(4):
            assert _mean(P, rows, 4, k, g0, 1) == rows[g0, k]
    assert _mean(P, rows, 4, 2, 1, 2) == (rows[1, 2] + rows[2, 2]) / 2  # (g0 and the stride: rows 1 and 2, column 2)


def test_mean_propagates_a_nan_row(P):
    rows = np.ones((5, 6))
    rows[3, 2] = np.nan
    assert np.isnan(_mean(P, rows, 6, 2, 0, 5)) and _mean(P, rows, 6, 1, 0, 5) == 1.0 and _mean(P, rows, 6, 2, 0, 3) == 1.0


def test_mean_sums_in_row_order(P):
    # 1e16 + 1 rounds back to 1e16: in row order the sum is 0, in any order that adds the two large terms first it is 1
    assert _mean(P, [1e16, 1.0, -1e16], 1, 0, 0, 3) == 0.0
    assert _mean(P, [1e16, -1e16, 1.0], 1, 0, 0, 3) == 1.0 / 3
    rng = np.random.default_rng(11)
    rows = rng.normal(size=(40, 4)) * 10.0 ** rng.integers(-8, 8, size=(40, 4))
    for k in range(4):
        s = 0.0
        for r in range(3, 40):
            s += rows[r, k]
        assert _mean(P, rows, 4, k, 3, 37) == s / 37
