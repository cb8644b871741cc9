"""Inputs and host references of the rollout bookkeeping tests (tests/test_rollout_cases_cpu.py, tests/test_gpu_rollout_ops.py): the case table of the
observation filter's batch push, a high-precision reference of its statistics (`ref_stats`: np.longdouble, two passes), a float64 restatement of the
kernel's own order of operations (`emulate_push`: what uhc_rollout.hip's uhc_filter_partial_kernel / uhc_filter_merge_kernel round, step by step), and
float64 restatements of uhc_filter_apply and uhc_rollout_record's bound.

Bounds (derived here, not from what the kernels give).  eps = 2^-53 * 2 = np.finfo(float64).eps.
  mean   |mean - ref| <= 8 eps * rms, rms = sqrt(ref_mean^2 + ref_S / n) the root mean square of the selected rows of the column.  (An error relative to
         |mean| alone has no meaning for a column that is centred on 0: a sum of n numbers of magnitude rms is uncertain by eps * rms whatever it adds up to.)
         Each level of the scheme -- 16-row sums, three merges of waves, merges of row blocks, the merge into the running triple -- adds about one rounding
         of a quantity of magnitude <= rms; the errors of different rows are independent, so 8 eps is several times what a correct implementation shows.
  S      |S - ref| <= 16 eps * (1 + max |mean| / std) * ref_S.  The deviations x - m are formed about the 16-row mean m, which carries eps * |mean| of
         rounding: relative to a deviation of size std that is eps * |mean| / std, squared deviations twice that; the 1 covers the roundings of the sums.
         Over the cases here the restated scheme uses at most 0.08 of this bound and 0.31 of the mean's (tests/test_rollout_cases_cpu.py prints both per case).
`emulate_push` rounds a multiply-add ONCE where the compiled kernel does (hipcc contracts `a * b + c` by default; read off the gfx950 code: S += w d d, and both
updates of a merge), which is what makes the device's mean and S equal it bit for bit; `fused=False` rounds twice and stays inside the same bounds.
The row-by-row Welford update (zfilter.py:17-27; `_welford` of the GPU test file) is 3 - 10 x FURTHER from `ref_stats` than this scheme: it is no yardstick here."""
import functools
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
ROWS_PER_BLOCK, ROWS_PER_WAVE = 64, 16  # FP_ROWS_PER_BLOCK, FP_ROWS_PER_WAVE of uhc_rollout.hip

ROW_EDGES = (1, 15, 16, 17, 63, 64, 65, 129, 4097)
DIM_EDGES = (1, 63, 64, 65, 1024, 1025, 1100)
LOC_SCALE = ((0.0, 1.0), (1e3, 1e-1), (1e6, 1e-2))
PATTERNS = ("none", "zero", "one", "wave", "block", "last")

# (n_rows, dim, (loc, scale), weight pattern of the second push).  Every row edge meets one narrow (<= 65) and one wide (>= 1024: the merge kernel's second
# trip over its 1024 threads starts at 1025) dim, every dim edge meets 65 rows (two row blocks, the second one row long), every pattern and every
# (loc, scale) occurs with several shapes.  Not the full product: 9 * 7 * 3 * 6 = 1134 cases would check nothing these do not.
FILTER_CASES = (
    (1, 1, LOC_SCALE[0], "none"), (1, 1024, LOC_SCALE[1], "one"),
    (15, 63, LOC_SCALE[1], "none"), (15, 1025, LOC_SCALE[0], "zero"),
    (16, 64, LOC_SCALE[2], "none"), (16, 1100, LOC_SCALE[0], "one"),
    (17, 65, LOC_SCALE[0], "wave"), (17, 1024, LOC_SCALE[1], "none"),
    (63, 1, LOC_SCALE[2], "wave"), (63, 1025, LOC_SCALE[0], "none"),
    (64, 63, LOC_SCALE[0], "wave"), (64, 1100, LOC_SCALE[2], "zero"),
    (65, 1, LOC_SCALE[1], "none"), (65, 63, LOC_SCALE[2], "block"), (65, 64, LOC_SCALE[0], "last"), (65, 65, LOC_SCALE[1], "one"),
    (65, 1024, LOC_SCALE[2], "wave"), (65, 1025, LOC_SCALE[1], "zero"), (65, 1100, LOC_SCALE[2], "last"),
    (129, 64, LOC_SCALE[1], "block"), (129, 1025, LOC_SCALE[2], "last"),
    (4097, 65, LOC_SCALE[2], "last"), (4097, 1100, LOC_SCALE[1], "block"),
)


def case_id(case):
    n_rows, dim, (loc, scale), pattern = case
    return f"{n_rows}x{dim}-loc{loc:g}-{pattern}"


def weights_of(pattern, n_rows, rng):
    """0/1 int32 weights of one push, or None (every row counts)."""
    if pattern == "none":
        return None
    w = np.ones(n_rows, dtype=np.int32)
    n_blocks = (n_rows + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK
    if pattern == "zero":
        w[:] = 0
    elif pattern == "one":  # exactly one row selected
        w[:] = 0
        w[int(rng.integers(n_rows))] = 1
    elif pattern == "wave":  # the rows of one whole wave deselected
        assert n_rows > ROWS_PER_WAVE
        k = int(rng.integers((n_rows + ROWS_PER_WAVE - 1) // ROWS_PER_WAVE))
        w[k * ROWS_PER_WAVE:(k + 1) * ROWS_PER_WAVE] = 0
    elif pattern == "block":  # one whole row block deselected
        assert n_blocks >= 2
        k = int(rng.integers(n_blocks - 1))
        w[k * ROWS_PER_BLOCK:(k + 1) * ROWS_PER_BLOCK] = 0
    elif pattern == "last":  # only the last, partial block selected
        assert n_blocks >= 2 and n_rows % ROWS_PER_BLOCK != 0
        w[:(n_blocks - 1) * ROWS_PER_BLOCK] = 0
    else:
        raise ValueError(pattern)
    return w


@functools.lru_cache(maxsize=None)
def filter_inputs(case):
    """(x1, None), (x2, w2): the two successive pushes of a case (read-only arrays, shared between the tests of a process)."""
    n_rows, dim, (loc, scale), pattern = case
    rng = np.random.default_rng([n_rows, dim, PATTERNS.index(pattern), int(loc)])
    x1 = loc + scale * rng.standard_normal((n_rows, dim))
    x2 = loc + scale * (0.5 + rng.standard_normal((n_rows, dim)))
    w2 = weights_of(pattern, n_rows, rng)
    for a in (x1, x2, w2):
        if a is not None:
            a.setflags(write=False)
    return (x1, None), (x2, w2)


# ---- A1: the high-precision reference ---------------------------------------------------------------------------------------------------------------
def ref_stats(chunks, weights):
    """(count, mean[dim], S[dim] = sum (x - mean)^2) over the selected rows of all chunks, in np.longdouble, two passes."""
    rows = [np.asarray(x, dtype=np.longdouble)[(slice(None) if w is None else np.asarray(w) != 0)] for x, w in zip(chunks, weights)]
    x = np.concatenate(rows, axis=0)
    n = x.shape[0]
    if n == 0:
        d = np.asarray(chunks[0]).shape[1]
        return 0, np.zeros(d, dtype=np.longdouble), np.zeros(d, dtype=np.longdouble)
    mean = x.sum(0) / np.longdouble(n)
    dev = x - mean
    return n, mean, (dev * dev).sum(0)


def stats_bounds(n, mean, S):
    """(absolute bound of the mean per column, absolute bound of S per column) for statistics whose reference is (n, mean, S)."""
    mean, S = np.asarray(mean, dtype=np.float64), np.asarray(S, dtype=np.float64)
    rms = np.sqrt(mean * mean + S / max(n, 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(S > 0, np.abs(mean) / np.sqrt(S / max(n - 1, 1)), 0.0)
    return 8 * EPS * rms, 16 * EPS * (1 + (ratio.max() if ratio.size else 0.0)) * S


# ---- A2: the kernel's order of operations in float64 ----------------------------------------------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    c = 134217729.0  # 2^27 + 1 (Dekker / Veltkamp)
    ah = c * a
    ah = ah - (ah - a)
    al = a - ah
    bh = c * b
    bh = bh - (bh - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """round(a * b + c) with ONE rounding, element-wise on float64 arrays, from float64 operations alone (Boldo & Melquiond, "Emulation of a FMA and
    correctly rounded sums", IEEE TC 2008: an exact product, two exact sums, one addition rounded to odd, one to nearest).  Valid where no intermediate
    over- or underflows, which holds for the magnitudes here (|x| <= 1e7, deviations >= 1e-12 or exactly 0).  The device compiler contracts `a * b + c`
    into v_fma_f64 wherever the source leaves it free to, so that is what the kernels round."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c)))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, ul)
    vh, vl = _two_sum(uh, th)
    z, err = _two_sum(tl, vl)  # ... rounded to odd: where inexact and the last bit of z is even, step towards the error
    z = np.array(z, dtype=np.float64)
    fix = (err != 0) & ((z.view(np.int64) & 1) == 0)
    z = np.where(fix, np.nextafter(z, np.where(err > 0, np.inf, -np.inf)), z)
    return vh + z


def _mul_add(a, b, c, fused):
    return fma(a, b, c) if fused else a * b + c


def chan_merge(na, ma, Sa, nb, mb, Sb, fused=True):
    """chan_merge of uhc_rollout.hip on arrays: counts broadcast against the columns; where nb == 0 the left side comes back untouched."""
    na, nb = np.asarray(na, dtype=np.float64), np.asarray(nb, dtype=np.float64)
    tot = na + nb
    with np.errstate(divide="ignore", invalid="ignore"):
        d = mb - ma
        S = _mul_add(d * d, na * nb / tot, Sa + Sb, fused)  # Sa + Sb + d * d * (na * nb / tot)
        m = _mul_add(d, nb / tot, ma, fused)  # ma + d * (nb / tot)
    skip = nb == 0
    return np.where(skip, na, tot), np.where(skip, ma, m), np.where(skip, Sa, S)


def emulate_push(x, w, n, M, S, fused=True):
    """uhc_filter_push on the host, in the kernel's order: every wave takes its <= 16 rows' weighted mean (sums in row order) and the squared deviations about
    it; the four waves of a row block are merged in wave order; the row blocks in block order; the result into the running (n, M, S).  Returns the new
    (n, M, S); the inputs are left alone.  fused: multiply-adds with one rounding where the compiled kernel has them (see `fma`)."""
    x = np.asarray(x, dtype=np.float64)
    n_rows, dim = x.shape
    M, S = np.array(M, dtype=np.float64), np.array(S, dtype=np.float64)
    if n_rows == 0:
        return float(n), M, S
    R = (n_rows + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK
    pad = R * ROWS_PER_BLOCK
    v = np.zeros((pad, dim))
    v[:n_rows] = x
    wt = np.zeros(pad)
    wt[:n_rows] = 1.0 if w is None else (np.asarray(w) != 0).astype(np.float64)
    v = v.reshape(R, 4, ROWS_PER_WAVE, dim)
    wt = wt.reshape(R, 4, ROWS_PER_WAVE, 1)
    c = np.zeros((R, 4, 1))
    s = np.zeros((R, 4, dim))
    for i in range(ROWS_PER_WAVE):
        c = c + wt[:, :, i]
        s = s + wt[:, :, i] * v[:, :, i]  # (the product is exact: fused or not, the same bits)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.where(c > 0, s / c, 0.0)
    Sw = np.zeros((R, 4, dim))
    for i in range(ROWS_PER_WAVE):
        d = v[:, :, i] - m
        Sw = _mul_add(wt[:, :, i] * d, d, Sw, fused)  # S += w * d * d
    nb, mb, Sb = c[:, 0], m[:, 0], Sw[:, 0]
    for k in range(1, 4):
        nb, mb, Sb = chan_merge(nb, mb, Sb, c[:, k], m[:, k], Sw[:, k], fused)
    na, ma, Sa = np.zeros(1), np.zeros(dim), np.zeros(dim)
    for r in range(R):
        na, ma, Sa = chan_merge(na, ma, Sa, nb[r], mb[r], Sb[r], fused)
    nn, M, S = chan_merge(np.array([float(n)]), M, S, na, ma, Sa, fused)
    return float(nn[0]), M, S


@functools.lru_cache(maxsize=None)
def filter_expected(case):
    """Per push of a case: ((n, M, S) of `emulate_push`, (n, mean, S) of `ref_stats`); computed once per process, read-only."""
    (x1, w1), (x2, w2) = filter_inputs(case)
    dim = x1.shape[1]
    e1 = emulate_push(x1, w1, 0.0, np.zeros(dim), np.zeros(dim))
    e2 = emulate_push(x2, w2, *e1)
    out = ((e1, ref_stats([x1], [w1])), (e2, ref_stats([x1, x2], [w1, w2])))
    for emu, ref in out:
        for a in emu[1:] + ref[1:]:
            a.setflags(write=False)
    return out


def ulp_distance(a, b):
    """Number of float64 values between a and b, element-wise (same-sign finite values or zeros)."""
    a, b = (np.ascontiguousarray(v, dtype=np.float64).view(np.int64) for v in (a, b))
    a, b = (np.where(v < 0, np.int64(-2 ** 63) - v, v) for v in (a, b))  # order the bit patterns like the values
    return np.abs(a - b)


# ---- uhc_filter_apply, restated ------------------------------------------------------------------------------------------------------------------------
def ref_apply(x, n, M, S, demean, destd, clip):
    """y = clip((x - M) / (std + 1e-8), +-clip) as the kernel forms it: var = S / (n - 1) for n > 1, else M^2; subtract, divide and sqrt are correctly rounded
    on both sides, so the bits are the same.  A NaN stays a NaN through the clip, as through np.clip / torch.clamp (zfilter.py:64)."""
    y = np.array(x, dtype=np.float64)
    M, S = np.asarray(M, dtype=np.float64), np.asarray(S, dtype=np.float64)
    with np.errstate(all="ignore"):
        if demean:
            y = y - M
        if destd:
            var = S / (n - 1.0) if n > 1.0 else M * M
            y = y / (np.sqrt(var) + 1e-8)
        if clip != 0.0:
            y = np.minimum(np.maximum(y, -clip), clip)
    return y


# ---- uhc_rollout_record's sums -------------------------------------------------------------------------------------------------------------------------
def record_sum_bound(values, n_env):
    """Absolute bound of one of the record kernel's sums against math.fsum: each of the 1024 threads adds its ceil(n_env / 1024) envs in turn, a tree of
    log2(1024) levels adds the threads, one more addition lands on the running total and one rounding is the reference's own:
    (ceil(log2 1024) + ceil(n_env / 1024) + 2) eps sum |x| (Higham, Accuracy and Stability of Numerical Algorithms, 4.2: depth of the summation tree times eps)."""
    return (math.ceil(math.log2(1024)) + math.ceil(n_env / 1024) + 2) * EPS * math.fsum(abs(float(v)) for v in values)
