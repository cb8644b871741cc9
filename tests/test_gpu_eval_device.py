"""GPU: evaluation on the device (uhc_amd/csrc/uhc_eval.hip through uhc_amd/eval_ops.py) -- the metrics kernel against the values recorded from the reference and
against compute_metrics on ragged records, the record kernel against a numpy restatement of eval_seqs' loop, and eval_seqs end to end with eval_build host / device."""
import copy
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["root_dist", "vel_dist", "accel_dist", "mpjpe_g", "pa_mpjpe", "mpjpe"]
SENTINEL = -7.0
STRIDE, FR_QPOS, FR_WBPOS = 584, 0, 151


def _reference(pred, gt, pj, gj):
    from uhc_amd.smpllib.smpl_eval import compute_metrics
    return compute_metrics(dict(pred=pred, gt=gt, pred_jpos=pj, gt_jpos=gj, fail_safe=False, percent=1))


def _record_of(rows, pred, pj, gt_frame, row_cap, nqh):
    """an eval_ops.Record holding the given row counts, pred arrays and bank indices (everything else zero)"""
    import torch
    from uhc_amd import eval_ops as EO
    rec = EO.Record(len(rows), row_cap, nqh, torch.device("cuda", 0))
    rec.rows.copy_(torch.tensor(rows, dtype=torch.int32))
    rec.pred_qpos.copy_(torch.from_numpy(pred))
    rec.pred_jpos.copy_(torch.from_numpy(pj))
    rec.gt_frame.copy_(torch.from_numpy(gt_frame))
    return rec


def _run_metrics(rec, bank):
    import torch
    from uhc_amd import eval_ops as EO
    rm = torch.full((rec.n_env, rec.row_cap, 6), SENTINEL, dtype=torch.float64, device=bank.device)
    cm = torch.full((rec.n_env, 6), SENTINEL, dtype=torch.float64, device=bank.device)
    _, _, bad = EO.metrics(rec, bank, row_metrics=rm, clip_means=cm, wait=True)
    return rm.cpu().numpy(), cm.cpu().numpy(), bad


def test_metrics_kernel_matches_the_values_recorded_from_the_reference():
    import torch
    g = np.load(os.path.join(ROOT, "tests", "golden", "g11_metrics.npz"))
    T = g["pred"].shape[0]
    assert T == 30
    bank = np.zeros((T, STRIDE))
    bank[:, FR_QPOS:FR_QPOS + 76], bank[:, FR_WBPOS:FR_WBPOS + 72] = g["gt"], g["gt_jpos"]
    rec = _record_of([T], g["pred"][None].copy(), g["pred_jpos"][None].copy(), np.arange(T, dtype=np.int64)[None], T, 76)
    rm, cm, bad = _run_metrics(rec, torch.from_numpy(bank).cuda())
    assert bad == 0
    for k, name in enumerate(NAMES):
        ref = g["m_" + name]
        print(name, "max |device - recorded| =", np.abs(rm[0, :len(ref), k] - ref).max())
        np.testing.assert_allclose(rm[0, :len(ref), k], ref, atol=1e-9, rtol=0, err_msg=name)
        assert (rm[0, len(ref):, k] == SENTINEL).all()
        np.testing.assert_allclose(cm[0, k], ref.mean(), atol=1e-9, rtol=0, err_msg=name)


def test_metrics_kernel_on_ragged_rows():
    import torch
    rng = np.random.default_rng(5)
    n_env, cap, nqh, n_frames = 5, 9, 99, 40
    rows = [0, 2, 3, 8, 9]
    bank = rng.normal(size=(n_frames, STRIDE))
    pred = rng.normal(size=(n_env, cap, nqh))
    gt_frame = rng.integers(0, n_frames, size=(n_env, cap)).astype(np.int64)
    pj = bank[gt_frame][:, :, FR_WBPOS:FR_WBPOS + 72] + 0.1 * rng.normal(size=(n_env, cap, 72))
    dbank = torch.from_numpy(bank).cuda()
    rec = _record_of(rows, pred, pj, gt_frame, cap, nqh)
    rm, cm, bad = _run_metrics(rec, dbank)
    assert bad == 0
    for e, T in enumerate(rows):
        if T == 0:
            assert (rm[e] == SENTINEL).all() and np.isnan(cm[e]).all()  # nothing to score: every slot untouched, every mean over an empty set
            continue
        gf = bank[gt_frame[e, :T]]
        ref = _reference(pred[e, :T], gf[:, FR_QPOS:FR_QPOS + 76], pj[e, :T], gf[:, FR_WBPOS:FR_WBPOS + 72])
        for k, name in enumerate(NAMES):
            n = len(ref[name])
            assert n == T - (1 if name == "vel_dist" else 2 if name == "accel_dist" else 0)
            np.testing.assert_allclose(rm[e, :n, k], ref[name], atol=1e-9, rtol=0, err_msg=f"env {e} {name}")
            assert (rm[e, n:, k] == SENTINEL).all(), (e, name)  # slots beyond numpy's lengths are left as they were
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")  # (np.mean of an empty array warns and gives the NaN asked for)
                np.testing.assert_allclose(cm[e, k], np.mean(ref[name]), atol=1e-9, rtol=0, err_msg=f"env {e} mean {name}")
    assert np.isnan(cm[1, 2]) and np.isfinite(np.delete(cm[1], 2)).all()  # the 2-row env: no acceleration row
    # two runs are bit-identical
    rm2, cm2, _ = _run_metrics(rec, dbank)
    assert rm.tobytes() == rm2.tobytes() and cm.tobytes() == cm2.tobytes()
    # gt_frame entries outside the bank: not followed, counted, and NaN in every output that would have read them
    rec.gt_frame[3, 4], rec.gt_frame[4, 0] = n_frames, -1
    rec.gt_frame[1, 5] = 10 ** 12  # (beyond the env's rows: never read, not counted)
    rm3, cm3, bad = _run_metrics(rec, dbank)
    assert bad == 2
    assert np.isnan(rm3[3, 4]).all() and np.isnan(rm3[4, 0]).all()
    expect = rm.copy()
    expect[3, 4], expect[4, 0] = np.nan, np.nan
    expect[3, 3, 1], expect[3, 3, 2], expect[3, 2, 2] = np.nan, np.nan, np.nan  # the velocity / acceleration differences that reach into row 4
    np.testing.assert_array_equal(rm3, expect)
    assert np.isnan(cm3[3]).all() and np.isnan(cm3[4]).all() and cm3[:3].tobytes() == cm[:3].tobytes()


# ---------------------------------------------------------------- the record kernel
def _script(rng, n_env, steps, nq, nbody):
    """states and step outputs of a scripted episode batch: [steps][2] states (before / after the step), done / percent / reward per step"""
    s = dict(q=rng.normal(size=(steps, 2, n_env, nq)), x=rng.normal(size=(steps, 2, n_env, nbody * 3)), reward=rng.random(size=(steps, n_env)),
             done=np.zeros((steps, n_env), dtype=np.int32), percent=rng.random(size=(steps, n_env)) * 0.9)
    s["alive0"] = np.array([0, 1, 1, 1, 1, 1, 1], dtype=np.int32)  # env 0: inactive from the start
    s["clip0"] = np.array([0, 100, 200, 300, 400, 500, 600], dtype=np.int64)
    s["len"] = np.array([50, 50, 50, 50, 50, 50, 2], dtype=np.int32)  # env 6: a 2-frame clip, the gt index stops at its last frame
    d, p = s["done"], s["percent"]
    d[0, 0], p[0, 0] = 1, 1.0                      # (env 0 is not alive: its flags are not looked at)
    d[0, 1], p[0, 1] = 1, 1.0                      # env 1: done at step 0
    d[0, 2] = d[1, 2] = d[2, 2] = 1; p[2, 2] = 1.0  # env 2: two fail-safe hits in a row (percent != 1), then the end of the clip
    d[5, 3], p[5, 3] = 1, 1.0                      # env 3: six rows before its six steps, the seventh at `done`: over the cap
    d[1, 5] = d[3, 5] = 1; p[3, 5] = 1.0           # env 5: one hit, goes on, ends
    d[1, 6], p[1, 6] = 1, 1.0
    # (env 4 runs on: six rows, still alive at the end)
    return s


def _restate(s, fail_safe, row_cap, nqh):
    """eval_seqs' host loop (uhc_amd/agents/agent_copycat.py) on the script, rows capped at row_cap"""
    n_env, steps = len(s["alive0"]), len(s["done"])
    alive = s["alive0"].astype(bool).copy()
    rows = [dict(pred=[], jpos=[], gt=[]) for _ in range(n_env)]
    rewards = [[] for _ in range(n_env)]
    fs, percent, overflow, tele_log = np.zeros(n_env, dtype=int), np.zeros(n_env), 0, []

    def append(e, t, ph):
        nonlocal overflow
        if len(rows[e]["gt"]) >= row_cap:
            overflow += 1
            return
        rows[e]["pred"].append(s["q"][t, ph, e, :nqh]); rows[e]["jpos"].append(s["x"][t, ph, e, 3:75])
        rows[e]["gt"].append(s["clip0"][e] + min(t, s["len"][e] - 1))

    for t in range(steps):
        for e in np.nonzero(alive)[0]:
            append(e, t, 0)
        done = s["done"][t].astype(bool) & alive
        tele = np.zeros(n_env, dtype=int)
        for e in np.nonzero(alive)[0]:
            rewards[e].append(s["reward"][t, e])
        for e in np.nonzero(done)[0]:
            append(e, t, 1)
            if fail_safe and s["percent"][t, e] != 1:
                fs[e], tele[e] = 1, 1
            else:
                alive[e], percent[e] = False, s["percent"][t, e]
        tele_log.append(tele)
    return rows, rewards, fs, percent, overflow, alive, tele_log


@pytest.mark.parametrize("nq,nqh,nbody", [(76, 76, 25), (113, 99, 27)])  # the hinge humanoid alone; ball joints plus two objects behind it
@pytest.mark.parametrize("fail_safe", [True, False])
def test_record_kernel_matches_the_host_loop(nq, nqh, nbody, fail_safe):
    import torch
    from uhc_amd import eval_ops as EO
    n_env, cap, steps = 7, 6, 6
    s = _script(np.random.default_rng(3), n_env, steps, nq, nbody)
    dev = torch.device("cuda", 0)
    rec = EO.Record(n_env, cap, nqh, dev)
    for t_ in (rec.pred_qpos, rec.pred_jpos, rec.rewards):
        t_.fill_(SENTINEL)
    rec.gt_frame.fill_(int(SENTINEL))
    alive = torch.from_numpy(s["alive0"].copy()).to(dev)
    clip0, lens = torch.from_numpy(s["clip0"]).to(dev), torch.from_numpy(s["len"]).to(dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tele_log = []
    for t in range(steps):
        EO.record(rec, 0, t, up(s["q"][t, 0]), up(s["x"][t, 0]), clip0, lens, alive)
        EO.record(rec, 1, t, up(s["q"][t, 1]), up(s["x"][t, 1]), clip0, lens, alive, done=up(s["done"][t]), reward=up(s["reward"][t]), percent=up(s["percent"][t]),
                  fail_safe=fail_safe)
        tele_log.append(rec.tele.cpu().numpy().copy())
    rows, rewards, fs, percent, overflow, alive_ref, tele_ref = _restate(s, fail_safe, cap, nqh)
    assert overflow == 1 and int(rec.overflow.item()) == 1
    n_rows = [len(r["gt"]) for r in rows]
    assert n_rows[0] == 0 and n_rows[1] == 2 and n_rows[3] == cap and (n_rows[2] == 6 if fail_safe else n_rows[2] == 2)
    np.testing.assert_array_equal(rec.rows.cpu().numpy(), n_rows)
    np.testing.assert_array_equal(rec.steps.cpu().numpy(), [len(r) for r in rewards])
    np.testing.assert_array_equal(rec.fail_safe.cpu().numpy(), fs)
    assert fs.sum() == (2 if fail_safe else 0) and alive_ref[4] and alive_ref.sum() == 1
    np.testing.assert_array_equal(rec.percent.cpu().numpy(), percent)
    np.testing.assert_array_equal(alive.cpu().numpy(), alive_ref.astype(np.int32))
    np.testing.assert_array_equal(np.array(tele_log), np.array(tele_ref))
    pq, pj, gf, rw = rec.pred_qpos.cpu().numpy(), rec.pred_jpos.cpu().numpy(), rec.gt_frame.cpu().numpy(), rec.rewards.cpu().numpy()
    for e in range(n_env):
        T, S = n_rows[e], len(rewards[e])
        if T:
            np.testing.assert_array_equal(pq[e, :T], np.array(rows[e]["pred"]))
            np.testing.assert_array_equal(pj[e, :T], np.array(rows[e]["jpos"]))
            np.testing.assert_array_equal(gf[e, :T], np.array(rows[e]["gt"]))
        np.testing.assert_array_equal(rw[e, :S], np.array(rewards[e]))
        # nothing is written beyond the rows of an env -- for env 3 that is: nothing past the cap, into env 4's first row
        assert (pq[e, T:] == SENTINEL).all() and (pj[e, T:] == SENTINEL).all() and (gf[e, T:] == int(SENTINEL)).all() and (rw[e, S:] == SENTINEL).all()
    assert gf[6, 1] == gf[6, 2] == 601  # min(t, len - 1)


# ---------------------------------------------------------------- end to end
def _agent(tmp_path):
    import torch
    from tests.test_gpu_agent import _cfg, _loader
    from uhc_amd.agents import agent_dict
    torch.set_default_dtype(torch.float64)
    cfg = _cfg(tmp_path, n_env=8, batch=8 * 4)
    agent = agent_dict[cfg.agent_name](cfg, torch.float64, torch.device("cuda", 0), data_loader=_loader(cfg, n=5))
    agent.optimize_policy(0, save_model=False)
    return agent


def _both_passes(agent):
    """eval_seqs with eval_build host, then device, from the same running-filter state (the reset observation is filtered with update=True)"""
    rs = agent.running_state.rs
    st = copy.deepcopy(rs.__getstate__())
    out = {}
    for build in ("host", "device"):
        rs._n = st["_n"]
        rs._M[...], rs._S[...] = st["_M"], st["_S"]
        rs._host_changed()
        agent.cfg.eval_build = build
        out[build] = agent.eval_seqs(list(agent.data_loader.data_keys), agent.data_loader)
        n_after = rs.n
        out[build + "_n"] = n_after
    agent.cfg.eval_build = "host"
    return out


def _assert_same(out, loader):
    from uhc_amd.smpllib.smpl_eval import compute_metrics
    host, dev = out["host"], out["device"]
    assert out["host_n"] == out["device_n"]  # the same filter updates
    assert list(host) == list(dev) == list(loader.data_keys)
    for k in host:
        h, d = host[k], dev[k]
        assert list(h) == list(d), (list(h), list(d))
        for name in h:
            a, b = np.asarray(h[name]), np.asarray(d[name])
            assert a.shape == b.shape and a.dtype == b.dtype, (k, name, a.shape, b.shape, a.dtype, b.dtype)
            if a.dtype == bool:
                assert (a == b).all(), (k, name)
            else:
                print(k, name, "max |host - device| =", float(np.abs(a - b).max()) if a.size else 0.0)
                np.testing.assert_allclose(b, a, atol=1e-9, rtol=0, err_msg=f"{k} {name}")
        assert type(h["fail_safe"]) is type(d["fail_safe"]) is bool
        # the device pass's metrics are compute_metrics of its OWN trajectories
        own = compute_metrics(d)
        for name in NAMES + ["succ"]:
            np.testing.assert_allclose(np.asarray(d[name], dtype=float), np.asarray(own[name], dtype=float), atol=1e-9, rtol=0, err_msg=f"{k} own {name}")


def test_eval_seqs_on_the_device_matches_the_host_path(tmp_path):
    agent = _agent(tmp_path)
    loader = agent.data_loader
    # ---- fail_safe off: no device -> host read in the step loop
    agent.cfg.fail_safe = False
    out = _both_passes(agent)
    _assert_same(out, loader)
    for k, res in out["device"].items():
        T = loader.get_sample_len_from_key(k)
        assert res["pred"].shape == (res["gt"].shape[0], 76) and res["pred_jpos"].shape[1] == res["gt_jpos"].shape[1] == 72
        assert 2 <= res["pred"].shape[0] <= T + 1 and len(res["reward"]) == res["pred"].shape[0] - 1 and not res["fail_safe"]
    # ---- fail_safe on, a termination threshold that ends clips early: teleports, and clips with more rows than frames
    for ev in agent._eval_envs.values():
        ev.close()
    agent._eval_envs = {}
    agent.cfg.fail_safe = True
    agent.cfg.cfg_dict["body_diff_thresh_test"] = 0.02
    out = _both_passes(agent)
    _assert_same(out, loader)
    hit = [k for k, res in out["device"].items() if res["fail_safe"] and res["pred"].shape[0] > loader.get_sample_len_from_key(k)]
    assert hit, {k: (res["fail_safe"], res["pred"].shape[0], loader.get_sample_len_from_key(k)) for k, res in out["device"].items()}
    agent.env.close()
