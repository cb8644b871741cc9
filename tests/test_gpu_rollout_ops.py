"""GPU: the rollout bookkeeping kernels (uhc_amd/csrc/uhc_rollout.hip, through the C-ABI) against the framework expressions they replace
and against the reference's row-by-row Welford filter; then a whole sampling pass with and without them; then each kernel at the edges of its tiling
against host references (tests/rollout_cases.py): np.longdouble statistics, a float64 restatement of the push's order of operations, numpy, math.fsum."""
import numpy as np
import pytest

from uhc_amd.sim import REDO_DROPPED, REDO_GENERAL, REDO_LARGE, REDO_PRIMAL, REDO_PRIMAL_CAP, REDO_SWEPT, REDO_WINDOWED

pytestmark = pytest.mark.gpu


def _welford(rows, n=0, M=None, S=None):
    """uhc/khrylib/utils/zfilter.py:17-27, one row at a time."""
    d = rows.shape[1]
    M = np.zeros(d) if M is None else M.copy()
    S = np.zeros(d) if S is None else S.copy()
    for x in rows:
        n += 1
        if n == 1:
            M[...] = x
        else:
            old = M.copy()
            M[...] = old + (x - old) / n
            S[...] = S + (x - old) * (x - M)
    return n, M, S


@pytest.mark.parametrize("n_rows,dim", [(1024, 657), (100, 70), (1, 5), (4096, 33)])
def test_filter_push_equals_row_by_row_welford(n_rows, dim):
    import torch
    from uhc_amd.khrylib.utils.zfilter import RunningStat
    rng = np.random.default_rng(n_rows + dim)
    x1 = rng.normal(loc=rng.normal(scale=3.0, size=dim), scale=rng.uniform(0.01, 2.0, size=dim), size=(n_rows, dim))
    x2 = rng.normal(loc=1.0, scale=0.5, size=(n_rows, dim))
    w = (rng.uniform(size=n_rows) < 0.3).astype(np.int32)
    rs = RunningStat((dim,))
    rs.push_batch(torch.from_numpy(x1).cuda())
    n, M, S = _welford(x1)
    assert rs.n == n
    np.testing.assert_allclose(rs.mean, M, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(rs._S, S, rtol=1e-11, atol=1e-12)
    rs.push_batch(torch.from_numpy(x2).cuda(), weights=torch.from_numpy(w).cuda())  # 0/1 weights: only those rows count
    n, M, S = _welford(x2[w != 0], n, M, S)
    assert rs.n == n
    np.testing.assert_allclose(rs.mean, M, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(rs._S, S, rtol=1e-11, atol=1e-12)
    rs.push_batch(torch.from_numpy(x2).cuda(), weights=torch.zeros(n_rows, dtype=torch.int32, device="cuda"))  # nothing selected: unchanged
    assert rs.n == n
    np.testing.assert_allclose(rs.mean, M, rtol=1e-12, atol=1e-13)
    # bit-reproducible
    a, b = RunningStat((dim,)), RunningStat((dim,))
    for r in (a, b):
        r.push_batch(torch.from_numpy(x1).cuda())
        r.push_batch(torch.from_numpy(x2).cuda(), weights=torch.from_numpy(w).cuda())
    assert np.array_equal(a.mean, b.mean) and np.array_equal(a._S, b._S)


def test_filter_apply_is_the_reference_expression_bit_for_bit():
    import torch
    from uhc_amd.khrylib.utils.zfilter import ZFilter
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.normal(scale=4.0, size=(257, 41))).cuda()
    for demean, destd, clip in [(True, True, 5.0), (True, False, 0.0), (False, True, 10.0)]:
        f = ZFilter((41,), demean=demean, destd=destd, clip=clip)
        f.rs.push_batch(x)
        y = f(x, update=False)  # library kernel
        ref = f._call_torch(x)  # the same filter through framework ops
        assert torch.equal(y, ref)
        t = torch.zeros(1, dtype=torch.long, device="cuda")
        out = torch.empty_like(x)
        assert f(x, update=False, out=out, step_counter=t) is out and torch.equal(out, ref) and int(t.item()) == 1
    g = ZFilter((41,))  # n = 1: std = |mean| (zfilter.py:45)
    g.rs.push_batch(x[:1])
    assert torch.equal(g(x, update=False), g._call_torch(x))


def test_act_and_record_equal_the_framework_expressions():
    import torch
    from uhc_amd import rollout_ops as ops
    torch.manual_seed(0)
    n_env, T, od, ad = 96, 5, 37, 11
    dev = "cuda"
    state = torch.randn(n_env, od, dtype=torch.float64, device=dev)
    mean = torch.randn(n_env, ad, dtype=torch.float64, device=dev)
    log_std = torch.randn(1, ad, dtype=torch.float64, device=dev) * 0.5 - 2.0
    noise = torch.randn(n_env, ad, dtype=torch.float64, device=dev)
    flags = (torch.rand(T, n_env, device=dev) < 0.4).double()
    states = torch.zeros(n_env, T, od, dtype=torch.float64, device=dev)
    actions = torch.zeros(n_env, T, ad, dtype=torch.float64, device=dev)
    action = torch.zeros(n_env, ad, dtype=torch.float64, device=dev)
    t = torch.full((1,), 3, dtype=torch.long, device=dev)
    ops.act(t, state, mean, log_std, noise, flags, states, actions, action)
    want = torch.where(flags[3].reshape(-1, 1).bool(), mean, mean + torch.exp(log_std.expand_as(mean)) * noise)
    # (exp of the library kernel and of the framework may differ in the last bit; everything else is the same arithmetic)
    assert float((action - want).abs().max()) < 1e-15 and torch.equal(actions[:, 3], action) and torch.equal(states[:, 3], state)
    assert torch.equal(action[flags[3] != 0], mean[flags[3] != 0])
    assert float(actions[:, :3].abs().max()) == 0.0 and float(states[:, 4].abs().max()) == 0.0
    # record
    reward = torch.rand(n_env, dtype=torch.float64, device=dev)
    done = (torch.rand(n_env, device=dev) < 0.2).int()
    end = (torch.rand(n_env, device=dev) < 0.1).int()
    parts = torch.rand(n_env, 6, dtype=torch.float64, device=dev)
    er = torch.full((), 2.5, dtype=torch.float64, device=dev)
    rewards = torch.zeros(n_env, T, dtype=torch.float64, device=dev)
    dones = torch.zeros(n_env, T, dtype=torch.float64, device=dev)
    crs = torch.full((), 1.0, dtype=torch.float64, device=dev)
    cis = torch.ones(5, dtype=torch.float64, device=dev)
    redo = torch.tensor([0, 1, 3, 0x70b, 0x80, 0xc1, 0x40000041, 0x60000041] * (n_env // 8) + [1] * (n_env % 8), dtype=torch.int32, device=dev)
    rc = torch.tensor([10, 20, 30, 40, 50, 60, 70], dtype=torch.long, device=dev)
    ops.record(t, reward, done, end, er, parts, 5, rewards, dones, crs, cis, redo, rc)
    assert rc.tolist() == [10 + int(((redo & REDO_GENERAL) != 0).sum()), 20 + int(((redo & REDO_SWEPT) != 0).sum()), 30 + int(((redo & REDO_DROPPED) != 0).sum()), 40 + int(((redo & REDO_LARGE) != 0).sum()), 50 + int(((redo & REDO_WINDOWED) != 0).sum()),
                           60 + int(((redo & REDO_PRIMAL) != 0).sum()), 70 + int(((redo & REDO_PRIMAL_CAP) != 0).sum())]  # (tier 4: solved by Newton on the primal; its iteration cap)
    assert torch.equal(rewards[:, 3], reward + end.double() * 2.5) and torch.equal(dones[:, 3], done.double())
    np.testing.assert_allclose(float(crs), 1.0 + float(reward.sum()), rtol=1e-14)
    np.testing.assert_allclose(cis.cpu().numpy(), 1.0 + parts[:, :5].sum(0).cpu().numpy(), rtol=1e-14)


def test_sampling_pass_with_and_without_the_library_bookkeeping(tmp_path, monkeypatch):
    """One sampling pass (graphs off, same seeds) through the library's bookkeeping kernels and through the framework ops: same batch.
    The two filters round differently in the last bits, the physics amplifies that a little over the pass."""
    import torch
    from tests.test_gpu_agent import _cfg, _loader
    from uhc_amd import rollout_ops
    from uhc_amd.agents import agent_dict
    torch.set_default_dtype(torch.float64)
    out = []
    for fused in (True, False):
        if not fused:
            monkeypatch.setattr(rollout_ops, "usable", lambda *a: False)
        torch.manual_seed(1)
        np.random.seed(1)
        cfg = _cfg(tmp_path, n_env=32, batch=32 * 6)
        agent = agent_dict[cfg.agent_name](cfg, torch.float64, torch.device("cuda", 0), data_loader=_loader(cfg))
        agent.use_graph = False
        agent.seed(5)
        batch, log = agent.sample(cfg.min_batch_size)
        out.append((batch.states.clone(), batch.actions.clone(), batch.rewards.clone(), batch.masks.clone(), agent.running_state.rs.n, log.avg_c_reward))
    a, b = out
    assert a[4] == b[4] and torch.equal(a[3], b[3])
    assert float((a[0] - b[0]).abs().max()) < 1e-7 and float((a[1] - b[1]).abs().max()) < 1e-7 and float((a[2] - b[2]).abs().max()) < 1e-7
    assert abs(a[5] - b[5]) < 1e-9


# ---- the kernels at their edges, against host references (tests/rollout_cases.py) -------------------------------------------------------------------------
from tests import rollout_cases as RC  # noqa: E402


def _bits_or_report(name, got, want):
    """Bit equality; a failure names the first column and the distance in units of the last place."""
    if np.array_equal(got, want):
        return
    d = RC.ulp_distance(got, want)
    col = int(np.argmax(d != 0))
    raise AssertionError(f"{name}: {int((d != 0).sum())} of {d.size} columns differ from the emulation, first column {col}: {got[col]!r} vs {want[col]!r} "
                         f"({int(d[col])} ulp), worst {int(d.max())} ulp")


@pytest.mark.parametrize("case", RC.FILTER_CASES, ids=RC.case_id)
def test_filter_push_at_the_edges_of_its_tiling(case):
    """uhc_filter_push, two successive pushes (the second weighted where the case has weights): the count exact, mean and S inside the bounds of the
    np.longdouble reference AND the bits of the float64 restatement of the kernel's order of operations; a push that selects no row changes no bit."""
    import torch
    from uhc_amd.khrylib.utils.zfilter import RunningStat
    n_rows, dim = case[0], case[1]
    pushes = RC.filter_inputs(case)
    zero = torch.zeros(n_rows, dtype=torch.int32, device="cuda")
    rs = RunningStat((dim,))
    rs.push_batch(torch.tensor(pushes[0][0], device="cuda"), weights=zero)  # a first-ever push with every row deselected
    assert rs.n == 0 and not rs.mean.any() and not rs._S.any()
    for (x, w), (emu, ref) in zip(pushes, RC.filter_expected(case)):
        rs.push_batch(torch.tensor(x, device="cuda"), weights=None if w is None else torch.tensor(w, device="cuda"))  # (torch.tensor copies: the inputs are read-only arrays)
        n, M, S = rs.n, rs.mean.copy(), rs._S.copy()
        assert n == ref[0] == emu[0]
        b_mean, b_S = RC.stats_bounds(*ref)
        e_mean = np.abs(M.astype(np.longdouble) - ref[1]).astype(np.float64)
        e_S = np.abs(S.astype(np.longdouble) - ref[2]).astype(np.float64)
        print(f"{RC.case_id(case)}: n {n}, worst error / bound: mean {np.max(e_mean / np.where(b_mean > 0, b_mean, 1)):.3f}, S {np.max(e_S / np.where(b_S > 0, b_S, 1)):.3f}")
        assert (e_mean <= b_mean).all() and (e_S <= b_S).all()
        _bits_or_report("mean", M, emu[1])
        _bits_or_report("S", S, emu[2])
    rs.push_batch(torch.tensor(pushes[1][0], device="cuda"), weights=zero)  # nothing selected: (n, M, S) bit-identical
    assert rs.n == n and np.array_equal(rs.mean, M) and np.array_equal(rs._S, S)


@pytest.mark.parametrize("n_rows", [1, 257])
@pytest.mark.parametrize("dim", [1, 65, 1025])
def test_filter_apply_equals_its_float64_restatement(n_rows, dim):
    """uhc_filter_apply against numpy (RC.ref_apply: subtract, divide and sqrt are correctly rounded on both sides, so the bits agree): every switch, clip = 0,
    n = 0 / 1 / 2 / many, a column without spread (S = 0: the divide is by 1e-8, then clipped), inputs at +-clip exactly, and a NaN that stays one NaN."""
    import torch
    from uhc_amd.khrylib.utils.zfilter import ZFilter
    rng = np.random.default_rng([n_rows, dim])
    M = rng.normal(scale=3.0, size=dim)
    S = rng.uniform(0.5, 40.0, size=dim)
    S[dim // 2] = 0.0
    x = M + rng.normal(scale=2.0, size=(n_rows, dim))
    x[0, 0] = 5.0  # at the clip bounds exactly, and their neighbours (reached as they are with demean = destd = False)
    x[-1, -1] = -5.0
    x[n_rows // 2, dim // 3] = np.nextafter(5.0, 6.0)
    xn = x.copy()
    xn[n_rows // 3, dim // 2] = np.nan
    for demean, destd, clip in [(True, True, 5.0), (True, False, 0.0), (False, True, 10.0), (True, True, 0.0), (False, False, 5.0)]:
        for n in (0, 1, 2, 1000):
            f = ZFilter((dim,), demean=demean, destd=destd, clip=clip)
            f.set_mean_std(M, S, n)
            for inp in (x, xn):
                got = f(torch.from_numpy(inp).cuda(), update=False).cpu().numpy()
                want = RC.ref_apply(inp, float(n), M, S, demean, destd, clip)
                assert np.array_equal(got, want, equal_nan=True), (demean, destd, clip, n)
                assert np.isnan(got).sum() == np.isnan(inp).sum()
            flat = got[:, dim // 2][np.isfinite(xn[:, dim // 2])]
            if clip and destd and n > 1:  # the column without spread: divided by 1e-8, then clipped
                assert (np.abs(flat) == clip).all()
            if clip and not demean and not destd:
                at = np.abs(x) >= 5.0
                assert at.any() and np.array_equal(got[at & np.isfinite(xn)], (np.sign(x) * 5.0)[at & np.isfinite(xn)])


def test_filter_apply_without_rows_still_counts_the_step():
    """n_rows = 0 with a step counter: the launch keeps one workgroup, whose first thread adds one to the counter and writes nothing else (the rollout's
    step index rides on this launch).  (A torch tensor without elements has no address, which the entry point refuses: the call goes through the C-ABI with
    the address of a tensor that has some.)"""
    import ctypes as C
    import torch
    from uhc_amd._lib import check, lib
    from uhc_amd import rollout_ops as ops
    dim = 7
    x = torch.full((4, dim), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((4, dim), float("nan"), dtype=torch.float64, device="cuda")
    n, M, S = torch.tensor(5.0, dtype=torch.float64, device="cuda"), torch.ones(dim, dtype=torch.float64, device="cuda"), torch.ones(dim, dtype=torch.float64, device="cuda")
    t = torch.full((1,), 41, dtype=torch.long, device="cuda")
    check(lib().uhc_filter_apply(ops._stream(x), ops._p(x), 0, dim, ops._p(n), ops._p(M), ops._p(S), 1, 1, C.c_double(5.0), ops._p(out), ops._p(t)))
    torch.cuda.synchronize()
    assert int(t.item()) == 42 and bool(torch.isnan(out).all()) and float(n) == 5.0 and bool((M == 1).all()) and bool((S == 1).all())
    with pytest.raises(Exception):
        ops.filter_apply(x[:0], n, M, S, True, True, 5.0, out[:0], t)  # no address: refused, and the counter stays
    assert int(t.item()) == 42


@pytest.mark.parametrize("n_env,obs_dim,act_dim", [(1, 0, 1), (3, 1, 1), (257, 37, 11), (1025, 5, 3)])
def test_act_against_the_host(n_env, obs_dim, act_dim):
    """uhc_rollout_act against numpy: flagged envs take the mean bit for bit; the others mean + exp(log_std) * noise with the product and the sum rounded
    separately, where the device's exp may be the neighbour of the correctly rounded one -- so each element equals one of three candidates, bit for bit.
    Only step t of the pass buffers is written; t = T and t = -1 write nothing at all."""
    import torch
    from uhc_amd import rollout_ops as ops
    T = 3
    rng = np.random.default_rng([n_env, obs_dim, act_dim])
    state, mean, noise = rng.normal(size=(n_env, obs_dim)), rng.normal(size=(n_env, act_dim)), rng.normal(size=(n_env, act_dim))
    log_std = rng.normal(size=(1, act_dim)) * 0.5 - 2.0
    flags = (rng.uniform(size=(T, n_env)) < 0.4).astype(np.float64)
    flags[:, ::2] = 1.0  # mixed wherever there are two envs ...
    flags[:, 1::2] = 0.0
    flags[T - 1, 0] = 0.0  # ... and over the steps where there is one
    e = np.exp(log_std.astype(np.longdouble)).astype(np.float64)
    cands = [mean + ee * noise for ee in (np.nextafter(e, 0.0), e, np.nextafter(e, np.inf))]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_state, d_mean, d_noise, d_log_std, d_flags = dev(state), dev(mean), dev(noise), dev(log_std), dev(flags)
    off_centre = 0
    for t in (0, T - 1, T, -1):
        states = torch.full((n_env, T, obs_dim), float("nan"), dtype=torch.float64, device="cuda")
        actions = torch.full((n_env, T, act_dim), float("nan"), dtype=torch.float64, device="cuda")
        action = torch.full((n_env, act_dim), float("nan"), dtype=torch.float64, device="cuda")
        ops.act(torch.full((1,), t, dtype=torch.long, device="cuda"), d_state, d_mean, d_log_std, d_noise, d_flags, states, actions, action)
        got, g_states, g_actions = action.cpu().numpy(), states.cpu().numpy(), actions.cpu().numpy()
        if not 0 <= t < T:
            assert np.isnan(got).all() and np.isnan(g_states).all() and np.isnan(g_actions).all()
            continue
        flagged = flags[t] != 0
        assert np.array_equal(got[flagged], mean[flagged])
        hit = np.stack([got == c for c in cands])
        assert hit[:, ~flagged].any(0).all(), f"t {t}: {(~hit[:, ~flagged].any(0)).sum()} elements equal no candidate; worst |difference| {np.abs(got - cands[1])[~flagged].max()}"
        off_centre += int((~hit[1][~flagged]).sum())
        assert np.array_equal(g_actions[:, t], got) and np.array_equal(g_states[:, t], state)
        others = [s for s in range(T) if s != t]
        assert np.isnan(g_actions[:, others]).all() and np.isnan(g_states[:, others]).all()
    print(f"act {n_env}x{obs_dim}+{act_dim}: {off_centre} elements took a neighbour of the correctly rounded exp")


@pytest.mark.parametrize("n_parts", [0, 5, 8])
@pytest.mark.parametrize("n_env", [1, 1023, 1024, 1025, 2500, 4096])
def test_record_against_the_host(n_env, n_parts):
    """uhc_rollout_record beyond one trip of its 1024 threads over the envs: rewards / dones of step t exact, the seven counts exact, the reward and part sums
    against math.fsum at the bound of the kernel's summation tree (RC.record_sum_bound), two launches the same bits, without the redo words no count
    moves, and a step outside the pass leaves every output alone."""
    import math
    import torch
    from uhc_amd import rollout_ops as ops
    T, t_in, stride = 3, 1, 9
    rng = np.random.default_rng([n_env, n_parts])
    reward = rng.uniform(size=n_env) * 10.0 ** rng.integers(-3, 3, size=n_env)
    done, end = (rng.uniform(size=n_env) < 0.3).astype(np.int32), (rng.uniform(size=n_env) < 0.2).astype(np.int32)
    parts = rng.uniform(-1.0, 1.0, size=(n_env, stride))
    bits = [REDO_GENERAL, REDO_SWEPT, REDO_DROPPED, REDO_LARGE, REDO_WINDOWED, REDO_PRIMAL, REDO_PRIMAL_CAP]
    redo = np.zeros(n_env, dtype=np.int64)
    for b in bits:
        redo |= np.where(rng.uniform(size=n_env) < 0.4, b, 0)
    known = 0
    for b in bits:
        known |= b
    redo |= rng.integers(0, 2 ** 31, size=n_env) & ~known & 0x7fffffff  # words the kernel does not count ride along
    redo = redo.astype(np.int32)
    er, crs0, cis0, rc0 = 2.5, 1.25, np.arange(1, 9, dtype=np.float64), np.array([10, 20, 30, 40, 50, 60, 70])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_reward, d_done, d_end, d_parts, d_redo, d_er = dev(reward), dev(done), dev(end), dev(parts), dev(redo), torch.full((), er, dtype=torch.float64, device="cuda")

    def launch(t, with_redo):
        rewards = torch.full((n_env, T), float("nan"), dtype=torch.float64, device="cuda")
        dones = torch.full((n_env, T), float("nan"), dtype=torch.float64, device="cuda")
        crs, cis, rc = torch.full((), crs0, dtype=torch.float64, device="cuda"), dev(cis0), dev(rc0)
        ops.record(torch.full((1,), t, dtype=torch.long, device="cuda"), d_reward, d_done, d_end, d_er, d_parts, n_parts, rewards, dones, crs, cis,
                   d_redo if with_redo else None, rc)
        return rewards.cpu().numpy(), dones.cpu().numpy(), float(crs), cis.cpu().numpy(), rc.cpu().numpy()

    for with_redo in (True, False):
        rewards, dones, crs, cis, rc = launch(t_in, with_redo)
        assert np.array_equal(rewards[:, t_in], reward + end * er) and np.array_equal(dones[:, t_in], done.astype(np.float64))
        assert np.isnan(rewards[:, [0, 2]]).all() and np.isnan(dones[:, [0, 2]]).all()
        assert rc.tolist() == ([int(c + ((redo & b) != 0).sum()) for c, b in zip(rc0, bits)] if with_redo else rc0.tolist())
        want = math.fsum([crs0] + list(reward))
        bound = RC.record_sum_bound([crs0] + list(reward), n_env)
        print(f"record {n_env} envs, {n_parts} parts: reward sum off by {abs(crs - want):.3e}, bound {bound:.3e}")
        assert abs(crs - want) <= bound
        for k in range(n_parts):
            col = [cis0[k]] + list(parts[:, k])
            assert abs(cis[k] - math.fsum(col)) <= RC.record_sum_bound(col, n_env), k
        assert np.array_equal(cis[n_parts:], cis0[n_parts:])  # terms beyond n_parts (and the stride's padding) are not summed
        again = launch(t_in, with_redo)
        assert np.array_equal(again[0], rewards, equal_nan=True) and again[2] == crs and np.array_equal(again[3], cis) and np.array_equal(again[4], rc)
    for t in (T, -1):
        rewards, dones, crs, cis, rc = launch(t, True)
        assert np.isnan(rewards).all() and np.isnan(dones).all() and crs == crs0 and np.array_equal(cis, cis0) and np.array_equal(rc, rc0)
