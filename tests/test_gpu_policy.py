"""GPU: the library's frozen policy (uhc_amd/csrc/uhc_policy.hip through uhc_amd/policy_ops.py): raw observations -> action means on v_mfma_f64_16x16x4_f64.

Values are compared with the torch modules in float64 on the CPU (which tests/golden/g12_policy_mcp.npz pins to the reference).  The tolerance is not fixed in
advance: in the same test torch's own device forward is measured against torch CPU on the same inputs (d_fw: the framework differing from itself under another
summation order and another erf), and the kernel gets max(4 d_fw, 1e-14) -- 4 because two independent roundings of the same length are compared, 1e-14
because that is the project's own bar for this golden on the CPU.  Bit-level properties are compared by equality."""
import copy
import gc
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
SHAPES = [(1, 1), (7, 12), (24, 19), (16, 4), (17, 5), (33, 17)]  # (out, in): the CPU list without its last shape
ROWS = [1, 15, 16, 17, 65]
ACTS = ["none", "tanh", "relu", "sigmoid", "gelu"]


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def _gaussian(state_dim, hsize, action_dim, htype, seed=0):
    import torch
    from uhc_amd.khrylib.models.mlp import _ACT
    from uhc_amd.khrylib.rl.core import PolicyGaussian
    torch.manual_seed(seed)
    pol = PolicyGaussian(types.SimpleNamespace(policy_hsize=list(hsize), policy_htype="tanh" if htype == "none" else htype, fix_std=True, log_std=-2.3),
                         action_dim=action_dim, state_dim=state_dim).double()
    if htype == "none":
        pol.net.activation = _identity
    pol.action_mean.bias.data.normal_(std=0.1)  # (the initial head has a zero bias: give the epilogue something to add)
    return pol


def _identity(x):
    return x


def _mcp_g12():
    import torch
    from uhc_amd.models.policy_mcp import PolicyMCP
    g = np.load(os.path.join(G, "g12_policy_mcp.npz"))
    pol = PolicyMCP(_Cfg(policy_hsize=[24, 16, 12], policy_htype="gelu", fix_std=True, log_std=-2.3, num_primitive=4, composer_dim=[20, 10]), action_dim=7, state_dim=19).double()
    pol.load_state_dict({k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("pol_")})  # (into float64 parameters: nothing is rounded)
    return pol, g


def _device_policy(pol, max_rows, running_state=None):
    """DevicePolicy of a module; an identity trunk (activation "none") goes through from_arrays, which is what from_modules calls"""
    from uhc_amd import policy_ops as PO
    if getattr(pol, "net", None) is not None and pol.net.activation is _identity:
        layers = [(l.weight.detach().numpy(), l.bias.detach().numpy(), PO.ACT_NONE) for l in list(pol.net.affine_layers) + [pol.action_mean]]
        dp = PO.DevicePolicy.from_arrays(PO.GAUSSIAN, layers[0][0].shape[1], [layers], max_rows=max_rows)
        if running_state is not None:
            dp.set_filter(running_state)
        return dp
    return PO.DevicePolicy.from_modules(pol, running_state, max_rows=max_rows)


def _figures(pol, x, got, what):
    """-> (the kernel's error, the tolerance): both against torch CPU on the same inputs; prints them with d_fw"""
    import torch
    with torch.no_grad():
        ref = pol(x).loc
        fw = copy.deepcopy(pol).cuda()(x.cuda()).loc.cpu()
    d_fw = float((fw - ref).abs().max())
    err = float((got.cpu() - ref).abs().max())
    tol = max(4.0 * d_fw, 1e-14)
    print(f"policy_act {what}: d_fw = {d_fw:.3e}  kernel error = {err:.3e}  tolerance = {tol:.3e}  max |mean| = {float(ref.abs().max()):.3e}")
    return err, tol


def _frozen_filter(dim, n=10, seed=4, **kw):
    from uhc_amd.khrylib.utils.zfilter import ZFilter
    rng = np.random.default_rng(seed)
    f = ZFilter((dim,), **kw)
    f.set_mean_std(rng.normal(scale=0.1, size=dim), rng.uniform(0.5, 2.0, size=dim) * 9, n)  # (mean, S, n)
    return f


# ------------------------------------------------------------------ exact data: a wrong lane map cannot pass
@pytest.mark.parametrize("out,inn", SHAPES)
def test_integer_data_gives_the_integer_product_bit_for_bit(out, inn):
    """two chained layers without activation, inn -> out -> 5: the packed weight, the A operand read from the caller's rows, the C / D -> next-A store and
    the row-major store of the last layer"""
    import torch
    from uhc_amd import policy_ops as PO
    rng = np.random.default_rng(out * 1000 + inn)
    W1, b1 = rng.integers(-3, 4, (out, inn)).astype(np.float64), rng.integers(-3, 4, out).astype(np.float64)
    W2, b2 = rng.integers(-3, 4, (5, out)).astype(np.float64), rng.integers(-3, 4, 5).astype(np.float64)
    dp = PO.DevicePolicy.from_arrays(PO.GAUSSIAN, inn, [[(W1, b1, PO.ACT_NONE), (W2, b2, PO.ACT_NONE)]], max_rows=max(ROWS))
    assert (dp.kind, dp.obs_dim, dp.act_dim, dp.max_rows, dp.n_primitives) == (PO.GAUSSIAN, inn, 5, 65, 0)
    for rows in ROWS:
        X = rng.integers(-3, 4, (rows, inn)).astype(np.float64)
        got = dp.mean(torch.from_numpy(X).cuda()).cpu().numpy()
        assert np.array_equal(got, (X @ W1.T + b1) @ W2.T + b2), (rows, out, inn)
    dp.close()


# ------------------------------------------------------------------ values
def test_g12_mcp_mean_and_composer_weight_match_the_golden():
    import torch
    pol, g = _mcp_g12()
    x = torch.from_numpy(g["x"])
    assert x.shape == (32, 19)
    dp = _device_policy(pol, 32)
    assert dp.n_primitives == 4 and dp.act_dim == 7
    w = torch.empty(32, 4, dtype=torch.float64, device="cuda")
    got = dp.mean(x.cuda(), weight_out=w)
    err, tol = _figures(pol, x, got, "g12 MCP 19 -> 24 -> 16 -> 12 -> 7 x 4, composer 19 -> 20 -> 10 -> 4, 32 rows")
    assert err <= tol
    with torch.no_grad():
        wref = pol.composer(x)
        wfw = copy.deepcopy(pol).cuda().composer(x.cuda()).cpu()
    werr, wtol = float((w.cpu() - wref).abs().max()), max(4.0 * float((wfw - wref).abs().max()), 1e-14)
    print(f"policy_act g12 composer weight: kernel error = {werr:.3e}  tolerance = {wtol:.3e}")
    assert werr <= wtol
    # ... and the recorded values themselves
    assert np.abs(got.cpu().numpy() - g["mean"]).max() <= max(tol, 1e-14) and np.abs(w.cpu().numpy() - g["weight"]).max() <= max(wtol, 1e-14)
    dp.close()


@pytest.mark.parametrize("htype", ACTS)
def test_gaussian_5_17_33_3_with_every_activation(htype):
    """hidden widths 17 and 33: no multiple of 4 (padding columns: sigmoid makes 0.5 of a zero there, which must contribute nothing) nor of 16"""
    import torch
    pol = _gaussian(5, [17, 33], 3, htype, seed=ACTS.index(htype))
    dp = _device_policy(pol, 65)
    torch.manual_seed(11)
    X = torch.randn(65, 5, dtype=torch.float64) * 2.0
    for rows in ROWS:
        got = dp.mean(X[:rows].cuda())
        err, tol = _figures(pol, X[:rows], got, f"Gaussian 5 -> 17 -> 33 -> 3 {htype}, {rows} rows")
        assert err <= tol, (htype, rows, err, tol)
    dp.close()


def test_full_size_gaussian_gelu_643_2048_1024_512_69():
    import torch
    pol = _gaussian(643, [2048, 1024, 512], 69, "gelu", seed=5)
    dp = _device_policy(pol, 48)
    torch.manual_seed(12)
    X = torch.randn(48, 643, dtype=torch.float64)
    got = dp.mean(X.cuda())
    err, tol = _figures(pol, X, got, "Gaussian 643 -> 2048 -> 1024 -> 512 -> 69 gelu, 48 rows")
    assert err <= tol
    dp.close()


# ------------------------------------------------------------------ bit-level properties
@pytest.fixture(scope="module", params=["gaussian", "mcp"])
def rig(request):
    """a policy with a filter set, 65 rows of observations and their means (computed once, left unchanged)"""
    import torch
    if request.param == "mcp":
        pol, _ = _mcp_g12()
    else:
        pol = _gaussian(5, [17, 33], 3, "gelu", seed=2)
    dim = 19 if request.param == "mcp" else 5
    filt = _frozen_filter(dim, clip=5)
    dp = _device_policy(pol, 65, filt)
    torch.manual_seed(13)
    X = (torch.randn(65, dim, dtype=torch.float64) * 2.0).cuda()
    full = dp.mean(X).clone()
    yield types.SimpleNamespace(pol=pol, filt=filt, dp=dp, X=X, full=full, dim=dim)
    dp.close()


def test_two_calls_give_identical_bits(rig):
    import torch
    assert torch.equal(rig.dp.mean(rig.X), rig.full) and torch.isfinite(rig.full).all()


def test_a_rows_bits_do_not_depend_on_the_batch_or_on_its_place_in_it(rig):
    import torch
    for r in (0, 20, 64):
        alone = rig.dp.mean(rig.X[r:r + 1])
        assert torch.equal(alone[0], rig.full[r]), r
    in17 = rig.dp.mean(rig.X[10:27])  # row 20 at place 10 of 17 rows
    assert torch.equal(in17, rig.full[10:27])
    perm = torch.randperm(65, generator=torch.Generator().manual_seed(1)).cuda()
    assert torch.equal(rig.dp.mean(rig.X[perm].contiguous()), rig.full[perm])  # every row at another place of 65


def test_a_view_into_a_wider_array_gives_the_bits_of_a_packed_copy(rig):
    import torch
    wide = torch.full((65, rig.dim + 4), 7.0, dtype=torch.float64, device="cuda")
    wide[:, 2:2 + rig.dim] = rig.X
    view = wide[:, 2:2 + rig.dim]
    assert view.stride(0) == rig.dim + 4 and not view.is_contiguous()
    assert torch.equal(rig.dp.mean(view), rig.full)


def test_a_nan_row_is_nan_and_leaves_every_other_row_alone(rig):
    import torch
    X = rig.X.clone()
    X[5, 2] = float("nan")
    state = torch.empty_like(X)
    got = rig.dp.mean(X, state_out=state)
    assert torch.isnan(got[5]).all()
    keep = torch.arange(65, device="cuda") != 5
    assert torch.equal(got[keep], rig.full[keep])
    assert torch.isnan(state[5, 2]) and torch.isfinite(state[keep]).all()


def test_the_filtered_result_matches_the_modules_behind_the_filter(rig):
    """the filter and the net together: against torch CPU on ZFilter(update=False)'s output"""
    import torch
    x = torch.from_numpy(rig.filt(rig.X.cpu().numpy(), update=False))
    err, tol = _figures(rig.pol, x, rig.full, f"{type(rig.pol).__name__} behind the filter, 65 rows")
    assert err <= tol


# ------------------------------------------------------------------ the filter
@pytest.mark.parametrize("n", [10, 1])
def test_state_out_has_the_bits_of_uhc_filter_apply(n):
    import torch
    from uhc_amd import rollout_ops
    pol = _gaussian(5, [17, 33], 3, "tanh", seed=3)
    dp = _device_policy(pol, 65)
    torch.manual_seed(14)
    X = (torch.randn(65, 5, dtype=torch.float64) * 8.0).cuda()  # (beyond the clip on both sides)
    state = torch.full_like(X, -7.0)
    dp.mean(X, state_out=state)
    assert torch.equal(state, X)  # no filter set: the observation as it is
    plain = dp.mean(X).clone()
    for demean in (False, True):
        for destd in (False, True):
            for clip in (0.0, 5.0):
                f = _frozen_filter(5, n=n, demean=demean, destd=destd, clip=clip)
                dp.set_filter(f)
                state = torch.full_like(X, -7.0)
                got = dp.mean(X, state_out=state)
                f.rs._to_device(X.device)
                want = torch.empty_like(X)
                rollout_ops.filter_apply(X, *f.rs._dev, demean, destd, clip, want)
                assert torch.equal(state, want), (n, demean, destd, clip)
                assert torch.isfinite(got).all() and (demean or destd or clip or torch.equal(got, plain))  # (all three off: the observation as it is)
                if clip:
                    assert float(state.abs().max()) <= 5.0
    dp.set_filter(None)
    assert torch.equal(dp.mean(X), plain)  # the filter taken off again
    dp.close()


# ------------------------------------------------------------------ edges
def test_row_count_edges_and_refusals():
    import ctypes as C
    import torch
    from uhc_amd._lib import UhcError, lib
    pol = _gaussian(5, [17, 33], 3, "relu", seed=6)
    big, dp = _device_policy(pol, 65), _device_policy(pol, 17)
    torch.manual_seed(15)
    X = torch.randn(18, 5, dtype=torch.float64).cuda()
    out = torch.full((0, 3), 1.0, dtype=torch.float64, device="cuda")
    assert dp.mean(X[:0], out=out).shape == (0, 3)  # n_rows = 0 succeeds
    assert lib().uhc_policy_act(None, dp._h, 0, None, 5, None, None, None) == 0
    assert torch.equal(dp.mean(X[:17]), big.mean(X)[:17])  # n_rows = max_rows
    with pytest.raises(UhcError, match=r"uhc_policy_act: n_rows = 18 is above the handle's max_rows = 17"):
        dp.mean(X)
    P = C.c_void_p
    assert lib().uhc_policy_act(None, dp._h, 4, P(X.data_ptr()), 4, None, P(X.data_ptr()), None) != 0
    assert lib().uhc_last_error().decode() == "uhc_policy_act: obs_stride = 4 is below obs_dim = 5"
    with pytest.raises(ValueError, match="weight_out"):
        dp.mean(X[:4], weight_out=torch.empty(4, 2, dtype=torch.float64, device="cuda"))
    with pytest.raises(NotImplementedError, match="mean actions only"):
        dp.select_action(X[:4], False)
    assert torch.equal(dp.select_action(X[:4]), dp.mean(X[:4]))
    big.close()
    dp.close()


@pytest.mark.parametrize("where", ["cuda", "cpu"])
def test_refresh_after_an_optimiser_step_matches_the_module_again(where):
    import torch
    pol = _gaussian(5, [17, 33], 3, "gelu", seed=7).to(where)
    from uhc_amd.policy_ops import DevicePolicy
    dp = DevicePolicy.from_modules(pol, max_rows=16)
    torch.manual_seed(16)
    X = torch.randn(16, 5, dtype=torch.float64)
    before = dp.mean(X.cuda()).clone()
    opt = torch.optim.SGD(pol.parameters(), lr=0.5)
    pol(X.to(where)).loc.square().sum().backward()
    opt.step()
    assert torch.equal(dp.mean(X.cuda()), before)  # frozen: the handle holds its own copy
    dp.refresh()
    after = dp.mean(X.cuda())
    err, tol = _figures(pol.cpu() if where == "cpu" else copy.deepcopy(pol).cpu(), X, after, f"after refresh from {where} modules")
    assert err <= tol and float((after - before).abs().max()) > 1e-3
    dp.close()


@pytest.mark.parametrize("kind", ["gaussian", "mcp"])
def test_save_and_load_give_the_same_action_bits(kind, tmp_path):
    import torch
    from uhc_amd.policy_ops import DevicePolicy
    pol = _mcp_g12()[0] if kind == "mcp" else _gaussian(5, [17, 33], 3, "sigmoid", seed=8)
    dim = 19 if kind == "mcp" else 5
    dp = _device_policy(pol, 17, _frozen_filter(dim, clip=5))
    path = tmp_path / "policy.bin"
    dp.save(path)
    raw = path.read_bytes()
    assert raw[:8] == b"UHCPOLCY" and np.frombuffer(raw[8:28], np.int32).tolist() == [1, dp.kind, dim, dp.act_dim, 5 if kind == "mcp" else 1]
    n_par = sum(p.numel() for n, p in pol.named_parameters() if n != "action_log_std")
    assert np.array_equal(np.sort(np.frombuffer(raw[-8 * n_par:], np.float64)), np.sort(np.concatenate([p.detach().numpy().ravel() for n, p in pol.named_parameters() if n != "action_log_std"])))
    back = DevicePolicy.load(path, max_rows=17)
    assert (back.kind, back.obs_dim, back.act_dim, back.n_primitives, back.packed_bytes) == (dp.kind, dp.obs_dim, dp.act_dim, dp.n_primitives, dp.packed_bytes)
    torch.manual_seed(17)
    X = (torch.randn(17, dim, dtype=torch.float64) * 3.0).cuda()
    s0, s1 = torch.empty_like(X), torch.empty_like(X)
    assert torch.equal(back.mean(X, state_out=s1), dp.mean(X, state_out=s0)) and torch.equal(s0, s1)
    back.save(tmp_path / "again.bin")
    assert (tmp_path / "again.bin").read_bytes() == raw  # the round trip is bit-exact
    with pytest.raises(RuntimeError, match="no modules"):
        back.refresh()
    # a filter that was set and taken off again leaves nothing behind in the file
    dp.set_filter(None)
    dp.save(tmp_path / "bare.bin")
    bare = (tmp_path / "bare.bin").read_bytes()
    n_nets = 5 if kind == "mcp" else 1
    flat = int(np.frombuffer(raw[28:28 + 4 * n_nets], np.int32).sum())  # (the layers of all nets)
    at = 8 + 4 * (5 + n_nets + 2 * flat)  # where the filter's four switch words lie: behind the magic, the five header words and the three tables
    assert np.frombuffer(bare[at:at + 16], np.int32).tolist() == [0, 0, 0, 0] and not any(bare[at + 16:at + 16 + 8 * (2 + 2 * dim)])
    assert np.frombuffer(raw[at:at + 16], np.int32).tolist() == [1, 1, 1, 0]
    again = DevicePolicy.load(tmp_path / "bare.bin", max_rows=17)
    again.save(tmp_path / "bare2.bin")
    assert (tmp_path / "bare2.bin").read_bytes() == bare
    assert torch.equal(again.mean(X, state_out=s1), dp.mean(X, state_out=s0)) and torch.equal(s0, X) and torch.equal(s1, X)
    with pytest.raises(ValueError, match="out must be"):
        dp.mean(X, out=torch.empty(17, dp.act_dim, dtype=torch.float64))  # (a tensor that is not on the handle's device)
    again.close()
    dp.close()
    back.close()


# ------------------------------------------------------------------ HIP graph
def test_a_captured_call_replays_on_new_observations_with_the_bits_of_an_eager_call(rig):
    import torch
    obs = rig.X.clone()
    out = torch.zeros(65, rig.full.shape[1], dtype=torch.float64, device="cuda")
    weight = torch.zeros(65, 4, dtype=torch.float64, device="cuda") if rig.dp.n_primitives else None
    rig.dp.mean(obs, out=out, weight_out=weight)  # (a first call outside the capture)
    torch.cuda.synchronize()
    gc.collect()  # no finaliser may free device memory while a stream is capturing
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rig.dp.mean(obs, out=out, weight_out=weight)
    new = torch.flip(rig.X, dims=[0]).contiguous() * 0.5
    obs.copy_(new)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    w2 = torch.zeros_like(weight) if weight is not None else None
    assert torch.equal(replayed, rig.dp.mean(new, weight_out=w2)) and not torch.equal(replayed, rig.full)
    assert weight is None or torch.equal(weight, w2)


# ------------------------------------------------------------------ the Python surface
def test_stream_tracker_with_the_device_policy_steps_two_live_envs(tmp_path):
    import torch
    from uhc_amd import sim as S
    from uhc_amd.envs.humanoid_im import VecHumanoidEnv
    from uhc_amd.stream import StreamTracker
    from uhc_amd.utils.config_utils.copycat_config import Config
    cfg = Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path))
    cfg.env_init_noise = 0.0
    env = VecHumanoidEnv(cfg, n_env=2, mode="test")
    pol = _gaussian(env.obs_dim, [64, 32], env.action_dim, "gelu", seed=9)
    filt = _frozen_filter(env.obs_dim, clip=5)
    stand = np.load(os.path.join(ROOT, "uhc_amd", "assets", "standing_neutral.npz"))["qpos"]
    assert stand.shape == (76,)
    head = torch.from_numpy(np.tile(stand, (2, 3, 1)))
    env.live_begin(8)
    tr = StreamTracker(env, pol.cuda(), filt, policy="device")
    assert tr.device_policy.max_rows == 2 and tr.device_policy.obs_dim == env.obs_dim
    obs = tr.begin(head).clone()
    qpos0 = env.sim.field(S.F_QPOS).clone()
    nxt = torch.from_numpy(np.tile(stand, (2, 1)))
    qpos, done = tr.step(nxt)
    x = torch.from_numpy(filt(obs.cpu().numpy(), update=False))
    err, tol = _figures(copy.deepcopy(pol).cpu(), x, tr._action, "StreamTracker(policy='device'), 2 live envs")
    assert err <= tol  # the action is where the two paths are compared: the simulation amplifies a last-bit difference
    assert torch.isfinite(qpos).all() and not torch.equal(qpos, qpos0)
    a0 = tr._action.data_ptr()
    tr.step(nxt)
    assert tr._action.data_ptr() == a0 and torch.isfinite(env.sim.field(S.F_QPOS)).all()  # one fixed action tensor
    env.live_end()
    env.close()


def test_eval_seqs_with_policy_build_device_returns_what_torch_returns(tmp_path):
    import torch
    from uhc_amd.agents import agent_dict
    from uhc_amd.data_loaders.dataset_amass_single import DatasetAMASSSingle
    from uhc_amd.data_loaders.synthetic import make_synthetic_amass
    from uhc_amd.utils.config_utils.copycat_config import Config
    torch.set_default_dtype(torch.float64)
    cfg = Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path))
    cfg.n_env, cfg.min_batch_size, cfg.num_optim_epoch, cfg.no_log = 2, 16, 1, True
    cfg.policy_hsize = cfg.value_hsize = [64, 32]
    cfg.eval_build = "device"
    specs = dict(cfg.data_specs)
    specs["file_path"] = "synthetic"
    dl = DatasetAMASSSingle(specs, "train", pickle_data=make_synthetic_amass(2, seed=4, t_range=(12, 14)))
    from uhc_amd.policy_ops import DevicePolicy
    agent = agent_dict[cfg.agent_name](cfg, torch.float64, torch.device("cuda", 0), data_loader=dl)
    key = list(dl.data_keys)[:1]
    out = {}
    for build in ("torch", "device"):
        cfg.policy_build = build
        out[build] = agent.eval_seqs(key, dl)[key[0]]
    cfg.policy_build = "torch"
    assert list(out["torch"]) == list(out["device"])
    for name in out["torch"]:
        a, b = np.asarray(out["torch"][name]), np.asarray(out["device"][name])
        assert a.dtype == b.dtype and a.ndim == b.ndim, name
    assert np.isfinite(out["device"]["pred"]).all() and len(out["device"]["pred"]) >= 2
    assert np.array_equal(out["device"]["pred"][0], out["torch"]["pred"][0])  # (the reset pose: before any action)
    # A second evaluation, after the weights and the filter have moved, goes through the SAME handle (uhc_policy_set_params and set_filter again: what every
    # later chunk and every evaluation between training epochs does): it then holds what a fresh handle of the agent's modules holds, bit for bit
    dp0 = agent._device_policies[1]
    obs = (torch.randn(1, agent.state_dim, dtype=torch.float64) * 2.0).cuda()
    stale = dp0.mean(obs).clone()
    with torch.no_grad():
        for prm in agent.policy_net.parameters():
            prm.mul_(1.25)
    rs = agent.running_state.rs
    agent.running_state.set_mean_std(np.asarray(rs.mean) + 0.05, np.asarray(rs._S) * 1.5, int(rs.n))
    cfg.policy_build = "device"
    again = agent.eval_seqs(key, dl)[key[0]]
    cfg.policy_build = "torch"
    assert agent._device_policies[1] is dp0 and list(again) == list(out["device"]) and np.isfinite(again["pred"]).all()
    fresh = DevicePolicy.from_modules(agent.policy_net, agent.running_state, max_rows=1)
    s0, s1 = torch.empty_like(obs), torch.empty_like(obs)
    assert torch.equal(dp0.mean(obs, state_out=s0), fresh.mean(obs, state_out=s1)) and torch.equal(s0, s1)
    assert not torch.equal(dp0.mean(obs), stale)
    fresh.close()
    # the file a C program deploys, from the same agent
    path = agent.export_policy(str(tmp_path / "policy.bin"))
    dp = DevicePolicy.load(path, max_rows=2)
    assert (dp.obs_dim, dp.act_dim) == (agent.state_dim, agent.action_dim)
    dp.close()
    agent.env.close()
