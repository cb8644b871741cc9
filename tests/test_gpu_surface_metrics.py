"""GPU: contact quality on the device (uhc_amd/csrc/uhc_surface.hip through uhc_amd/eval_ops.py) -- the surface kernel against smpl_eval's host functions on the
CPU test's cases and on ragged records, read through the pose-record layout and through the clip bank's; uhc_eval_record_pose beside uhc_eval_record;
eval_seqs with eval_surface on under both builds; the expert clips of a device-built bank."""
import copy
import os
import warnings

import numpy as np
import pytest

from tests import surface_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-9  # mm
GUARD = 3    # guard rows in front of and behind every output array
LAYOUTS = {"record": (168, 0, 72), "bank": (584, 151, 223)}  # row stride, offset of the positions, of the quaternions (doubles)


def _rows_in_layout(pos, quat, layout):
    """pos [n][B][3], quat [n][B][4] -> device rows of the layout's stride, NaN wherever the kernel has no business reading"""
    import torch
    stride, op, oq = LAYOUTS[layout]
    n, B = pos.shape[0], pos.shape[1]
    buf = np.full((n, stride), np.nan)
    buf[:, op:op + 3 * B] = pos.reshape(n, -1)
    buf[:, oq:oq + 4 * B] = quat.reshape(n, -1)
    d = torch.from_numpy(buf).cuda()
    return d[:, op:op + 3 * B], d[:, oq:oq + 4 * B]


def _run(surface, pos, quat, seq_start, seq_rows, cap, layout="record", seq_model=None, floor_z=0.0):
    """-> (rows [n][4], means [n_seq][4], bad); the guard rows around both outputs must come back untouched"""
    import torch
    from uhc_amd import eval_ops as EO
    n, n_seq = pos.shape[0], len(seq_start)
    dp, dq = _rows_in_layout(pos, quat, layout)
    full = torch.full((n + 2 * GUARD, 4), SC.SENTINEL, dtype=torch.float64, device="cuda")
    mfull = torch.full((n_seq + 2 * GUARD, 4), SC.SENTINEL, dtype=torch.float64, device="cuda")
    sm = None if seq_model is None else torch.tensor(seq_model, dtype=torch.int32, device="cuda")
    _, _, bad = EO.surface_metrics(surface, dp, dq, torch.tensor(seq_start, dtype=torch.int64, device="cuda"), torch.tensor(seq_rows, dtype=torch.int32, device="cuda"),
                                   row_cap=cap, seq_model=sm, floor_z=floor_z, row_out=full[GUARD:GUARD + n], seq_means=mfull[GUARD:GUARD + n_seq], wait=True)
    full, mfull = full.cpu().numpy(), mfull.cpu().numpy()
    for g in (full[:GUARD], full[GUARD + n:], mfull[:GUARD], mfull[GUARD + n_seq:]):
        assert (g == SC.SENTINEL).all(), "a guard row was written"
    return full[GUARD:GUARD + n], mfull[GUARD:GUARD + n_seq], bad


def _surface_of(c):
    from uhc_amd import eval_ops as EO
    r = c["vert_radius"] if c["vert_radius"] is not None else np.zeros(c["V"])
    return EO.Surface([(v, c["vert_body"], r) for v in c["vert"]], n_body=SC.N_BODY)


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("kind", SC.KINDS)
def test_kernel_matches_the_host_functions_on_the_cpu_cases(kind):
    for V in SC.VERTS:
        for T in SC.ROWS:
            c = SC.make_case(kind, V, T)
            exp_rows, exp_means, exp_bad = SC.expected(c)
            S = _surface_of(c)
            got = {}
            for layout in LAYOUTS:
                rows, means, bad = _run(S, c["pos"], c["quat"], [0], [T], T, layout, seq_model=[c["model"]], floor_z=c["floor_z"])
                SC.assert_rows_match(rows, means[0], exp_rows, exp_means, (kind, V, T, layout), atol=ATOL)
                assert bad == exp_bad, (kind, V, T, layout)
                got[layout] = rows.tobytes() + means.tobytes()
            assert got["record"] == got["bank"], (kind, V, T)  # the same bits through either layout
            if kind == "models":  # a model index outside the range reads as model 0
                r0, _, _ = _run(S, c["pos"], c["quat"], [0], [T], T, seq_model=[0])
                for m in (-1, 2):
                    assert _run(S, c["pos"], c["quat"], [0], [T], T, seq_model=[m])[0].tobytes() == r0.tobytes()
                assert r0.tobytes() != got["record"][:r0.nbytes]
            S.close()


def _ragged(rng, V=130, cap=9, n_seq=5):
    vert = rng.uniform(-0.3, 0.3, size=(1, V, 3))
    body = rng.integers(0, SC.N_BODY, size=V).astype(np.int32)
    quat = rng.normal(size=(n_seq * cap, SC.N_BODY, 4))
    quat /= np.linalg.norm(quat, axis=-1, keepdims=True)
    pos = rng.uniform(-1.0, 1.0, size=(n_seq * cap, SC.N_BODY, 3))
    pos[:, :, 2] = rng.uniform(-0.1, 0.1, size=(n_seq * cap, SC.N_BODY))
    c = dict(kind="ragged", V=V, T=n_seq * cap, vert=vert, vert_body=body, vert_radius=None, pos=pos, quat=quat, floor_z=0.0, model=0, nan_row=None)
    SC.assert_clear_of_the_floor(c)
    return c


def _expected_ragged(c, seq_start, seq_rows, cap):
    """the host functions sequence by sequence: (rows [n][4] with SENTINEL where nothing is written, means [n_seq][4])"""
    rows, means = np.full((c["pos"].shape[0], 4), SC.SENTINEL), np.full((len(seq_start), 4), SC.SENTINEL)
    for s, (g0, T) in enumerate(zip(seq_start, seq_rows)):
        T = min(max(T, 0), cap)
        sub = dict(c, T=T, pos=c["pos"][g0:g0 + T], quat=c["quat"][g0:g0 + T])
        if T:
            rows[g0:g0 + T], means[s], _ = SC.expected(sub)
        else:
            means[s] = np.nan  # every mean over an empty set
    return rows, means


def test_kernel_on_ragged_records_in_both_layouts():
    from uhc_amd import eval_ops as EO
    cap, seq_rows = 9, [0, 1, 2, 8, 9]
    seq_start = [cap * s for s in range(5)]
    c = _ragged(np.random.default_rng(41), cap=cap)
    S = _surface_of(c)
    exp_rows, exp_means = _expected_ragged(c, seq_start, seq_rows, cap)
    got = {}
    for layout in LAYOUTS:
        rows, means, bad = _run(S, c["pos"], c["quat"], seq_start, seq_rows, cap, layout)
        assert bad == 0
        np.testing.assert_allclose(rows, exp_rows, atol=ATOL, rtol=0, err_msg=layout)
        np.testing.assert_array_equal(rows == SC.SENTINEL, exp_rows == SC.SENTINEL)  # slots beyond each length still hold the sentinel
        np.testing.assert_array_equal(rows[:, 3], exp_rows[:, 3])
        np.testing.assert_allclose(means, exp_means, atol=ATOL, rtol=0, equal_nan=True, err_msg=layout)
        got[layout] = rows.tobytes() + means.tobytes()
    assert got["record"] == got["bank"]
    assert np.isnan(exp_means[0]).all() and np.isnan(exp_means[1, 1]) and np.isfinite(np.delete(exp_means[1], 1)).all()  # no row; one row: no pair
    # two runs are bit-identical
    rows2, means2, _ = _run(S, c["pos"], c["quat"], seq_start, seq_rows, cap)
    assert rows2.tobytes() + means2.tobytes() == got["record"]
    # a row counter of -3 reads as no row, one of cap + 5 as cap rows: nothing is written outside the arrays (the guard rows are checked by _run)
    odd = [-3, 1, 2, 8, cap + 5]
    rows3, means3, bad = _run(S, c["pos"], c["quat"], seq_start, odd, cap)
    assert bad == 0 and rows3.tobytes() == rows.tobytes() and np.array_equal(means3, means, equal_nan=True)
    # a NaN row, and a sequence whose rows would leave 0 .. n_rows_total: counted, the sequence skipped
    pos = c["pos"].copy()
    pos[3 * cap + 4, 1, 0] = np.nan
    for start4 in (4 * cap + 1, -1, 2 ** 40):
        rows4, means4, bad = _run(S, pos, c["quat"], seq_start[:4] + [start4], seq_rows, cap)
        assert bad == 2, start4
        e = exp_rows.copy()
        e[4 * cap:] = SC.SENTINEL  # the skipped sequence: nothing of it is written
        e[3 * cap + 4] = np.nan
        e[3 * cap + 3, 1] = np.nan
        np.testing.assert_allclose(rows4, e, atol=ATOL, rtol=0, equal_nan=True)
        assert (means4[4] == SC.SENTINEL).all() and np.isnan(means4[3]).all() and means4[:3].tobytes() == means[:3].tobytes()
    # the two refusals that need a real handle: a stride below a row's width
    import torch
    z = torch.zeros(4, 8, dtype=torch.float64, device="cuda")
    for pos_v, quat_v, name in ((z[:, :6].as_strided((4, 6), (5, 1)), z, "pos_stride"), (z, z.as_strided((4, 8), (7, 1)), "quat_stride")):
        with pytest.raises(Exception, match=name):
            EO.surface_metrics(S, pos_v, quat_v, torch.zeros(1, dtype=torch.int64, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda"), row_cap=1)
    S.close()


# ---------------------------------------------------------------- record_pose beside record
@pytest.mark.parametrize("fail_safe", [True, False])
def test_record_pose_writes_the_rows_record_appends(fail_safe):
    import torch
    from tests.test_gpu_eval_device import _script
    from uhc_amd import eval_ops as EO
    n_env, cap, steps, nq, nqh, nbody = 7, 6, 6, 113, 99, 27
    rng = np.random.default_rng(3)
    s = _script(rng, n_env, steps, nq, nbody)  # envs that are dead from the start, done, hit by the fail-safe, and one that runs into the row cap
    xq = rng.normal(size=(steps, 2, n_env, nbody * 4))
    dev = torch.device("cuda", 0)
    rec = EO.Record(n_env, cap, nqh, dev, poses=True)
    rec.pred_pose.fill_(SC.SENTINEL)
    alive = torch.from_numpy(s["alive0"].copy()).to(dev)
    clip0, lens = torch.from_numpy(s["clip0"]).to(dev), torch.from_numpy(s["len"]).to(dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for t in range(steps):
        EO.record_pose(rec, 0, up(s["x"][t, 0]), up(xq[t, 0]), alive)
        EO.record(rec, 0, t, up(s["q"][t, 0]), up(s["x"][t, 0]), clip0, lens, alive)
        done = up(s["done"][t])
        EO.record_pose(rec, 1, up(s["x"][t, 1]), up(xq[t, 1]), alive, done=done)
        EO.record(rec, 1, t, up(s["q"][t, 1]), up(s["x"][t, 1]), clip0, lens, alive, done=done, reward=up(s["reward"][t]), percent=up(s["percent"][t]), fail_safe=fail_safe)
    # the selection rule, restated: alive, and (before the step, or done after it), and a row left
    live = s["alive0"].astype(bool).copy()
    want = [[] for _ in range(n_env)]
    for t in range(steps):
        for e in np.nonzero(live)[0]:
            if len(want[e]) < cap:
                want[e].append((t, 0))
        for e in np.nonzero(s["done"][t].astype(bool) & live)[0]:
            if len(want[e]) < cap:
                want[e].append((t, 1))
            if not (fail_safe and s["percent"][t, e] != 1):
                live[e] = False
    n_rows = rec.rows.cpu().numpy()
    np.testing.assert_array_equal(n_rows, [len(w) for w in want])
    assert n_rows[0] == 0 and n_rows[3] == cap and int(rec.overflow.item()) == 1
    pose, pj = rec.pred_pose.cpu().numpy(), rec.pred_jpos.cpu().numpy()
    for e in range(n_env):
        T = n_rows[e]
        for r, (t, ph) in enumerate(want[e]):
            np.testing.assert_array_equal(pose[e, r, :72], s["x"][t, ph, e, 3:75])
            np.testing.assert_array_equal(pose[e, r, 72:], xq[t, ph, e, 4:100])
        np.testing.assert_array_equal(pose[e, :T, :72], pj[e, :T])  # pose row r belongs to pred_qpos / pred_jpos row r
        assert (pose[e, T:] == SC.SENTINEL).all()  # nothing beyond the rows: for env 3 nothing past the cap, into env 4's first row
    with pytest.raises(ValueError, match="poses"):
        EO.record_pose(EO.Record(n_env, cap, nqh, dev), 0, up(s["x"][0, 0]), up(xq[0, 0]), alive)


# ---------------------------------------------------------------- end to end
TODAY = ["gt", "pred", "gt_jpos", "pred_jpos", "reward", "percent", "fail_safe", "root_dist", "vel_dist", "accel_dist", "mpjpe_g", "pa_mpjpe", "mpjpe", "succ"]


def _passes(agent, keep=None):
    """eval_seqs with eval_build host, then device, from the same running-filter state (tests/test_gpu_eval_device.py: _both_passes)"""
    rs = agent.running_state.rs
    st = copy.deepcopy(rs.__getstate__())
    out = {}
    for build in ("host", "device"):
        rs._n = st["_n"]
        rs._M[...], rs._S[...] = st["_M"], st["_S"]
        rs._host_changed()
        agent.cfg.eval_build = build
        out[build] = agent.eval_seqs(list(agent.data_loader.data_keys), agent.data_loader)
    agent.cfg.eval_build = "host"
    return out


def test_eval_seqs_scores_the_surface_on_both_builds(tmp_path, monkeypatch):
    from tests.test_gpu_eval_device import _agent
    from uhc_amd.smpllib import smpl_eval as E
    agent = _agent(tmp_path)
    agent.cfg.fail_safe = False
    # ---- off (the default): exactly today's dictionaries on both builds
    assert agent.cfg.eval_surface is False
    out = _passes(agent)
    for build in ("host", "device"):
        for res in out[build].values():
            assert list(res) == TODAY, (build, list(res))
    # ---- on
    agent.cfg.eval_surface = True
    seen = []  # the vertices the host pass scores, clip by clip
    real = E.hull_vertices
    monkeypatch.setattr(E, "hull_vertices", lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    out = _passes(agent)
    monkeypatch.undo()
    host, dev = out["host"], out["device"]
    assert list(host) == list(dev) and len(seen) == len(host)
    n_rows = n_out = 0
    for (k, h), vert in zip(host.items(), seen):
        d = dev[k]
        assert list(h) == list(d) == TODAY + ["pentration", "skate", "float", "contact"], (list(h), list(d))
        np.testing.assert_array_equal(d["pred"], h["pred"])  # the same trajectory
        near = np.abs(vert[:, :, 2]).min(axis=1) < 1e-9  # rows in which a vertex lies within 1e-9 m of the floor: their predicates may differ
        n_rows += len(near)
        assert h["contact"].shape == d["contact"].shape == near.shape and d["contact"].dtype == np.float64
        np.testing.assert_array_equal(d["contact"][~near], h["contact"][~near], err_msg=k)
        if near.any():  # the clip's means contain such a row: the clip is left out, and all its rows count as left out
            n_out += len(near)
            continue
        for name in ("pentration", "skate", "float"):
            assert np.ndim(d[name]) == 0 and np.ndim(h[name]) == 0
            print(k, name, "host", float(h[name]), "|host - device| =", abs(float(h[name]) - float(d[name])))
            np.testing.assert_allclose(d[name], h[name], atol=ATOL, rtol=0, err_msg=f"{k} {name}")
        assert (h["contact"] > 0).any()  # the humanoid stands on the floor
    print(f"rows left out of the comparison: {n_out} of {n_rows}")
    assert n_out <= 0.01 * n_rows
    # ---- eval_policy's means now carry the two reference metrics
    agent.cfg.eval_build = "device"
    (name, m), = agent.eval_policy(0)[0].items()
    assert np.isfinite(m["pentration"]) and np.isfinite(m["skate"]) and "float" not in m
    agent.cfg.eval_build = "host"
    agent.env.close()


# ---------------------------------------------------------------- the expert clips themselves
def test_surface_metrics_of_a_device_built_bank_match_the_host_functions():
    import torch
    from uhc_amd import eval_ops as EO
    from uhc_amd import sim as S
    from uhc_amd.sim import load_asset_model
    from uhc_amd.smpllib import smpl_eval as E
    from uhc_amd.smpllib.torch_smpl_humanoid import Humanoid
    model = load_asset_model()
    z = np.load(os.path.join(ROOT, "uhc_amd", "assets", "standing_neutral.npz"))
    rng = np.random.default_rng(9)
    lens = [1, 2, 7]
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    n = sum(lens)
    qpos = np.tile(z["qpos"], (n, 1))
    qpos[:, 7:] += rng.normal(scale=0.1, size=(n, qpos.shape[1] - 7))
    qpos[:, :2] += np.cumsum(rng.normal(scale=0.01, size=(n, 2)), axis=0)
    qpos[:, 2] += rng.uniform(-0.03, 0.03, size=n)  # clips that sink into the floor and clips that hover above it
    frames = S.expert_frames_device(torch.from_numpy(qpos), list(starts), [Humanoid(model=model)], device=torch.device("cuda", 0))
    surface = EO.Surface(model)
    rows, means, bad = EO.surface_metrics_of_bank(surface, frames, starts, lens, wait=True)
    assert bad == 0
    rows, means, fr = rows.cpu().numpy(), means.cpu().numpy(), frames.cpu().numpy()
    info = {"floor_z": 0}
    some_pen = some_float = False
    for s0, T, mean in zip(starts, lens, means):
        f = fr[s0:s0 + T]
        vert = E.hull_vertices(model, f[:, 151:223], f[:, 223:319])
        assert np.abs(vert[:, :, 2]).min() > 1e-9
        pen, skate, flo, con = E.compute_penetration(vert, info), E.compute_skate(vert, info), E.compute_float(vert, info), E.compute_contact(vert, info)
        np.testing.assert_allclose(rows[s0:s0 + T, 0], pen, atol=ATOL, rtol=0)
        np.testing.assert_allclose(rows[s0:s0 + T - 1, 1], skate, atol=ATOL, rtol=0)
        assert np.isnan(rows[s0 + T - 1, 1])  # the last row has no skate: the slot keeps what it held
        np.testing.assert_allclose(rows[s0:s0 + T, 2], flo, atol=ATOL, rtol=0)
        np.testing.assert_array_equal(rows[s0:s0 + T, 3], con)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            np.testing.assert_allclose(mean, [np.mean(pen), np.mean(skate), np.mean(flo), np.mean(con)], atol=ATOL, rtol=0, equal_nan=True)
        some_pen, some_float = some_pen or max(pen) > 0, some_float or max(flo) > 0
    assert some_pen and some_float
    surface.close()
