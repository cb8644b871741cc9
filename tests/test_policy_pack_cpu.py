"""CPU: the arithmetic uhc_policy.hip shares with the host (uhc_amd/csrc/uhc_policy_math.h, compiled with the host compiler: tests/policy_pack_probe.cpp) --
the packing is a bijection onto the non-padding slots, a host emulation of the tiled product built from the same lane maps equals the naive product exactly on
small-integer data through two chained layers, the activations and the filter's rule at their edges -- and what of the feature needs no device: the refusal
list of uhc_policy_create (every check comes before the first HIP call), the config key, the Python surface."""
import ctypes as C
import inspect
import math
import os
import types

import numpy as np
import pytest

from tests import probe_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (7, 12), (24, 19), (16, 4), (17, 5), (33, 17), (2048, 643)]  # (out, in)
ROWS = [1, 15, 16, 17, 65]
NONE, TANH, RELU, SIGMOID, GELU = range(5)
D, I, PD = C.c_double, C.c_int, C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(PD)


@pytest.fixture(scope="module")
def probe():
    L = C.CDLL(probe_build.build_probe("policy_pack_probe.so", ["tests/policy_pack_probe.cpp"], ["uhc_amd/csrc/uhc_policy_math.h"],
                                       ("-Wall", "-Werror", *probe_build.NO_CONTRACT)))
    for f in ("pol_w_index", "pol_x_index"):
        getattr(L, f).argtypes, getattr(L, f).restype = [I, I, I], C.c_int64
    for f in ("pol_w_doubles", "pol_x_doubles"):
        getattr(L, f).argtypes, getattr(L, f).restype = [I, I], C.c_int64
    L.pol_act.argtypes, L.pol_act.restype = [I, D], D
    L.pol_filter_denom.argtypes, L.pol_filter_denom.restype = [D, D, D], D
    L.pol_filter.argtypes, L.pol_filter.restype = [D, D, D, I, I, D], D
    L.pol_pack.argtypes, L.pol_pack.restype = [PD, PD, I, I, PD, PD], None
    L.pol_layer.argtypes, L.pol_layer.restype = [I, PD, I, I, PD, PD, I, I, I, PD], None
    return L


def _pack(L, W, b):
    N, K = W.shape
    wp = np.full(L.pol_w_doubles(N, K), np.nan)
    bp = np.full((N + 15) // 16 * 16, np.nan)
    L.pol_pack(_p(W), _p(b), N, K, _p(wp), _p(bp))
    return wp, bp


@pytest.mark.parametrize("out,inn", SHAPES)
def test_packing_is_a_bijection_onto_the_non_padding_slots_and_the_padding_is_zero(probe, out, inn):
    kpad, npad = (inn + 3) // 4 * 4, (out + 15) // 16 * 16
    assert probe.pol_w_doubles(out, inn) == npad * kpad
    W = np.arange(1, out * inn + 1, dtype=np.float64).reshape(out, inn)  # every element its own non-zero value
    b = -np.arange(1, out + 1, dtype=np.float64)
    wp, bp = _pack(probe, W, b)
    if out * inn <= 1 << 12:
        idx = np.array([[probe.pol_w_index(n, k, kpad) for k in range(inn)] for n in range(out)])
    else:  # the closed form the header states, checked against the compiled function on the small shapes and on a sample here
        n, k = np.meshgrid(np.arange(out), np.arange(inn), indexing="ij")
        idx = ((n >> 4) * (kpad >> 2) + (k >> 2)) * 64 + (k & 3) * 16 + (n & 15)
        for nn, kk in [(0, 0), (out - 1, inn - 1), (17, 5), (1000, 641), (2047, 3)]:
            assert idx[nn, kk] == probe.pol_w_index(nn, kk, kpad)
    assert idx.min() >= 0 and idx.max() < wp.size and np.unique(idx).size == out * inn  # injective, inside
    assert np.array_equal(wp[idx], W)  # the slot the map names holds the element
    rest = np.ones(wp.size, bool)
    rest[idx.ravel()] = False
    assert rest.sum() == npad * kpad - out * inn and np.all(wp[rest] == 0.0)  # ... and every other slot is an exact zero
    assert np.array_equal(bp[:out], b) and np.all(bp[out:] == 0.0)
    # the activation's map: the same bijection over (row, k)
    for rows in (1, 17):
        xi = np.array([[probe.pol_x_index(r, k, kpad) for k in range(min(inn, 40))] for r in range(rows)])
        assert xi.min() >= 0 and xi.max() < probe.pol_x_doubles(rows, inn) and np.unique(xi).size == xi.size


@pytest.mark.parametrize("out,inn", SHAPES)
def test_the_tiled_product_through_the_lane_maps_equals_the_naive_product_exactly(probe, out, inn):
    """two chained layers: (inn -> out, packed for the next layer) then (out -> 5, row-major): the output order of one is the input order of the next"""
    rng = np.random.default_rng(out * 1000 + inn)
    W1, b1 = rng.integers(-3, 4, (out, inn)).astype(np.float64), rng.integers(-3, 4, out).astype(np.float64)
    W2, b2 = rng.integers(-3, 4, (5, out)).astype(np.float64), rng.integers(-3, 4, 5).astype(np.float64)
    wp1, bp1 = _pack(probe, W1, b1)
    wp2, bp2 = _pack(probe, W2, b2)
    k4 = (out + 3) // 4 * 4

    def x_index(r, k):
        """the closed form uhc_policy_math.h states for the packed activation, for index arrays; checked against the compiled function below"""
        return ((r >> 4) * (k4 >> 2) + (k >> 2)) * 64 + (k & 3) * 16 + (r & 15)

    for r, k in [(0, 0), (15, out - 1), (16, 0), (64, out - 1), (79, k4 - 1), (33, out // 2)]:
        assert x_index(r, k) == probe.pol_x_index(r, k, k4), (r, k)
    if out <= 64:  # ... and element by element where that is quick
        assert all(x_index(r, k) == probe.pol_x_index(r, k, k4) for r in range(80) for k in range(k4))
    for rows in ROWS:
        X = rng.integers(-3, 4, (rows, inn)).astype(np.float64)
        mid = np.full(probe.pol_x_doubles(rows, out), np.nan)
        probe.pol_layer(1, _p(X), rows, inn, _p(wp1), _p(bp1), out, NONE, 0, _p(mid))
        assert np.isfinite(mid).all()  # every slot of the live row tiles was written
        H = X @ W1.T + b1
        rr, kk = np.meshgrid(np.arange(rows), np.arange(out), indexing="ij")
        idx = x_index(rr, kk)
        assert idx.min() >= 0 and idx.max() < mid.size and np.unique(idx).size == idx.size
        assert np.array_equal(mid[idx], H)  # the intermediate lies in the order the next layer reads
        rest = np.ones(mid.size, bool)
        rest[idx.ravel()] = False
        pr, pk = np.meshgrid(np.arange(rows, (rows + 15) // 16 * 16), np.arange(k4), indexing="ij")
        rest[x_index(pr, pk).ravel()] = False  # (rows beyond the batch hold the bias: never read back)
        assert rest.sum() == rows * (k4 - out) and np.all(mid[rest] == 0.0)  # the padding columns
        Y = np.full((rows, 5), np.nan)
        probe.pol_layer(0, _p(mid), rows, out, _p(wp2), _p(bp2), 5, NONE, 1, _p(Y))
        ref = H @ W2.T + b2
        assert np.abs(ref).max() < 2 ** 52 and np.array_equal(Y, ref), (rows, np.abs(Y - ref).max())


def test_padding_columns_stay_zero_under_an_activation_that_does_not_keep_zero(probe):
    # sigmoid(0) = 0.5: a hidden width that is no multiple of 4 leaves padding columns, which must be exact zeros in the next layer's operand
    rng = np.random.default_rng(1)
    W, b = rng.normal(size=(17, 5)), rng.normal(size=17)
    wp, bp = _pack(probe, W, b)
    X = rng.normal(size=(3, 5))
    mid = np.full(probe.pol_x_doubles(3, 17), np.nan)
    probe.pol_layer(1, _p(X), 3, 5, _p(wp), _p(bp), 17, SIGMOID, 0, _p(mid))
    for r in range(3):
        got = np.array([mid[probe.pol_x_index(r, k, 20)] for k in range(20)])
        np.testing.assert_allclose(got[:17], 1.0 / (1.0 + np.exp(-(X[r] @ W.T + b))), rtol=1e-15, atol=0)
        assert np.all(got[17:] == 0.0)


def test_activations_at_zero_tiny_large_and_nan(probe):
    tiny, large = 5e-324, 1e300
    for code in (NONE, TANH, RELU, SIGMOID, GELU):
        assert math.isnan(probe.pol_act(code, float("nan"))), code  # relu too: a comparison, not fmax
    assert probe.pol_act(99, 1.5) == 1.5  # (create refuses unknown codes; the function itself is the identity for them)
    assert [probe.pol_act(c, 0.0) for c in range(5)] == [0.0, 0.0, 0.0, 0.5, 0.0]
    assert probe.pol_act(NONE, -large) == -large and probe.pol_act(NONE, tiny) == tiny
    assert probe.pol_act(TANH, large) == 1.0 and probe.pol_act(TANH, -large) == -1.0 and probe.pol_act(TANH, tiny) == tiny and probe.pol_act(TANH, -tiny) == -tiny
    assert probe.pol_act(RELU, large) == large and probe.pol_act(RELU, -large) == 0.0 and probe.pol_act(RELU, tiny) == tiny and probe.pol_act(RELU, -tiny) == 0.0
    assert probe.pol_act(SIGMOID, large) == 1.0 and probe.pol_act(SIGMOID, -large) == 0.0 and probe.pol_act(SIGMOID, tiny) == 0.5 and probe.pol_act(SIGMOID, -tiny) == 0.5
    assert probe.pol_act(GELU, large) == large and probe.pol_act(GELU, -large) == 0.0 and abs(probe.pol_act(GELU, tiny)) <= tiny and abs(probe.pol_act(GELU, -tiny)) <= tiny
    # the exact erf form, not the tanh approximation (they differ by 2e-4 at 1.5)
    for v in (-2.0, -0.3, 0.7, 1.5):
        assert abs(probe.pol_act(GELU, v) - 0.5 * v * (1.0 + math.erf(v / math.sqrt(2.0)))) < 1e-15
        assert abs(probe.pol_act(SIGMOID, v) - 1.0 / (1.0 + math.exp(-v))) < 1e-16 and probe.pol_act(TANH, v) == math.tanh(v)


def test_filter_rule_at_n_0_1_2_and_at_S_0(probe):
    from uhc_amd.khrylib.utils.zfilter import ZFilter
    for n in (0, 1, 2, 10):
        for mean, S in ((0.25, 0.0), (-1.5, 3.0), (0.0, 0.0), (2.0, 1e-30)):
            want = (math.sqrt(S / (n - 1)) if n > 1 else abs(mean)) + 1e-8
            got = probe.pol_filter_denom(float(n), mean, S)
            assert got == want, (n, mean, S)
            for demean in (0, 1):
                for destd in (0, 1):
                    for clip in (0.0, 5.0):
                        f = ZFilter((1,), demean=bool(demean), destd=bool(destd), clip=clip)
                        f.set_mean_std(np.array([mean]), np.array([S]), n)
                        for x in (0.3, -40.0, 1e9, 0.0):
                            assert probe.pol_filter(x, mean, got, demean, destd, clip) == f(np.array([x]), update=False)[0], (n, mean, S, demean, destd, clip, x)
    assert math.isnan(probe.pol_filter(float("nan"), 0.1, 1.0, 1, 1, 5.0))  # the clip keeps a NaN


# ------------------------------------------------------------------ uhc_policy_create's refusals: before the first HIP call, so without a device
@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from uhc_amd import _lib
    return _lib.lib()


def _create(L, kind, obs_dim, act_dim, max_rows, nets, bad=None):
    """nets: [[(out, act), ...] per net]; weights of ones (bad = (flat layer, value): one entry of that layer's weight replaced) -> (rc, message)"""
    flat = [la for net in nets for la in net]
    w, b, i = [], [], 0
    for net in nets:
        k = obs_dim
        for out, _ in net:
            w.append(np.ones((max(out, 1), max(k, 1))))
            b.append(np.zeros(max(out, 1)))
            if bad is not None and bad[0] == i:
                w[-1][0, 0] = bad[1]
            k, i = out, i + 1
    I32 = C.c_int32
    h = C.c_void_p()
    rc = L.uhc_policy_create(kind, obs_dim, act_dim, max_rows, len(nets), (I32 * len(nets))(*[len(n) for n in nets]), (I32 * len(flat))(*[o for o, _ in flat]),
                             (I32 * len(flat))(*[a for _, a in flat]), (C.c_void_p * len(flat))(*[x.ctypes.data for x in w]),
                             (C.c_void_p * len(flat))(*[x.ctypes.data for x in b]), C.byref(h))
    return rc, L.uhc_last_error().decode(), h


def test_create_refuses_by_name_before_the_first_hip_call(capi):
    prim = [(8, GELU), (6, GELU), (3, NONE)]
    comp = [(5, GELU), (2, GELU)]
    cases = [
        ((0, 0, 3, 4, [prim]), "non-positive dimension"),
        ((0, 5, -1, 4, [prim]), "non-positive dimension"),
        ((0, 5, 3, 0, [prim]), "non-positive dimension"),
        ((0, 5, 3, 4, [[(8, GELU), (0, GELU), (3, NONE)]]), "non-positive dimension"),
        ((0, 5, 3, 4, [[(8, 5), (3, NONE)]]), "unknown activation"),
        ((0, 5, 3, 4, [[(8, -1), (3, NONE)]]), "unknown activation"),
        ((1, 5, 3, 4, [prim, [(8, GELU), (7, GELU), (3, NONE)], comp]), "primitives of unequal shape"),
        ((1, 5, 3, 4, [prim, [(8, GELU), (6, TANH), (3, NONE)], comp]), "primitives of unequal shape"),
        ((1, 5, 3, 4, [prim, [(8, GELU), (3, NONE)], comp]), "primitives of unequal shape"),
        ((1, 5, 3, 4, [prim, prim, [(5, GELU), (3, GELU)]]), "the composer's last width is not the number of primitives"),
        ((7, 5, 3, 4, [prim]), "unknown kind"),
    ]
    for args, text in cases:
        rc, msg, h = _create(capi, *args)
        assert rc != 0 and msg == "uhc_policy_create: " + text and not h.value, (args, msg)
    for value in (float("nan"), float("inf")):
        rc, msg, h = _create(capi, 1, 5, 3, 4, [prim, prim, comp], bad=(7, value))
        assert rc != 0 and msg == "uhc_policy_create: non-finite weight" and not h.value, msg
    # the other entries refuse a NULL handle and a bad row count / stride the same way
    P = C.c_void_p
    assert capi.uhc_policy_act(None, None, 1, None, 5, None, None, None) != 0 and capi.uhc_last_error().decode() == "uhc_policy_act: NULL policy"
    assert capi.uhc_policy_set_filter(None, 1.0, None, None, 1, 1, 0.0) != 0 and capi.uhc_last_error().decode() == "uhc_policy_set_filter: NULL policy"
    h = P()
    assert capi.uhc_policy_load(b"/nonexistent/policy.bin", 4, C.byref(h)) != 0 and "cannot open" in capi.uhc_last_error().decode() and not h.value


def test_load_refuses_a_file_that_is_not_a_policy(capi, tmp_path):
    h = C.c_void_p()
    for name, data, text in (("short", b"UHC", "not a policy file"), ("magic", b"NOTPOLCY" + bytes(64), "not a policy file"),
                             ("version", b"UHCPOLCY" + np.array([2, 0, 5, 3, 1], np.int32).tobytes(), "unknown file version"),
                             ("cut", b"UHCPOLCY" + np.array([1, 0, 5, 3, 1, 2], np.int32).tobytes(), "truncated file"),
                             ("dims", b"UHCPOLCY" + np.array([1, 0, -5, 3, 1, 2], np.int32).tobytes(), "bad header"),
                             # a header that asks for more than the file holds is refused before anything is sized from it: 16 MB of filter, 25 GB of weights
                             ("wide", b"UHCPOLCY" + np.array([1, 0, 1 << 20, 3, 1, 1, 3, 0, 0, 0, 0, 0], np.int32).tobytes() + bytes(64), "truncated file"),
                             ("deep", b"UHCPOLCY" + np.array([1, 0, 2, 3, 1, 3, 1 << 20, 1 << 20, 3, 0, 0, 0, 0, 0, 0, 0], np.int32).tobytes() + bytes(8 * 6 + 4096),
                              "truncated file")):
        path = tmp_path / name
        path.write_bytes(data)
        assert capi.uhc_policy_load(str(path).encode(), 4, C.byref(h)) != 0 and not h.value
        assert capi.uhc_last_error().decode() == "uhc_policy_load: " + text, name


def test_config_key_and_python_surface(tmp_path):
    import yaml
    from uhc_amd.agents.agent_copycat import AgentCopycat
    from uhc_amd.policy_ops import DevicePolicy
    from uhc_amd.stream import StreamTracker
    from uhc_amd.utils.config_utils.copycat_config import Config
    shipped = yaml.safe_load(open(os.path.join(ROOT, "config", "uhc_amd", "copycat_mi355x.yml")))
    assert Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path)).policy_build == "torch"
    assert Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path), cfg_dict=dict(shipped, policy_build="device")).policy_build == "device"
    with pytest.raises(ValueError, match="policy_build"):
        Config(cfg_id="copycat_mi355x", base_dir=str(tmp_path), cfg_dict=dict(shipped, policy_build="hip"))
    p = inspect.signature(StreamTracker.__init__).parameters
    assert list(p) == ["self", "env", "policy_net", "running_state", "dtype", "policy"] and p["policy"].default == "torch"
    with pytest.raises(ValueError, match="'torch' or 'device'"):
        StreamTracker(types.SimpleNamespace(n_env=1, device="cpu"), None, policy="hip")
    assert list(inspect.signature(DevicePolicy.from_modules).parameters)[:3] == ["policy_net", "running_state", "max_rows"]
    assert list(inspect.signature(DevicePolicy.mean).parameters) == ["self", "obs", "out", "state_out", "weight_out"]
    for name in ("refresh", "save", "load", "select_action", "set_filter"):
        assert callable(getattr(DevicePolicy, name))
    assert callable(AgentCopycat.export_policy)
    # anything but the two policies is refused with its class name, before a device is touched
    import torch
    from uhc_amd.khrylib.models.mlp import MLP
    from uhc_amd.khrylib.rl.core import Value
    with pytest.raises(TypeError, match="Value"):
        DevicePolicy.from_modules(Value(MLP(5, [4], "tanh")))
    with pytest.raises(TypeError, match="Linear"):
        DevicePolicy.from_modules(torch.nn.Linear(3, 2))
