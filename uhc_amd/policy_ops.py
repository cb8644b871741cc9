"""Host side of the frozen policy of the library (uhc_amd/csrc/uhc_policy.hip; C-ABI in include/uhc_amd.h: uhc_policy_*): a trained `PolicyGaussian` or
`PolicyMCP` and its observation filter as ONE call from raw observations to action means -- depth (+ 1 for MCP) launches of the library instead of the
framework's chain of filter, addmm, activation and copy launches.  Device float64 only.  Mean actions only: sampling stays with `rollout_ops.act`; the
training sampler, whose filter statistics move every step, the value net and the backward pass stay with the framework (DESIGN)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import check, lib

GAUSSIAN, MCP = 0, 1
ACT_NONE, ACT_TANH, ACT_RELU, ACT_SIGMOID, ACT_GELU = range(5)


def _act_code(fn):
    if isinstance(fn, torch.nn.GELU):
        if getattr(fn, "approximate", "none") != "none":
            raise ValueError("DevicePolicy: nn.GELU(approximate='tanh') is not the exact erf form the library computes")
        return ACT_GELU
    for f, code in ((torch.tanh, ACT_TANH), (torch.relu, ACT_RELU), (torch.sigmoid, ACT_SIGMOID)):
        if fn is f:
            return code
    raise ValueError(f"DevicePolicy: unknown activation {fn!r}")


def _nets_of(policy_net):
    """-> (kind, [[(nn.Linear, activation code), ...] per net]): the primitives, then the composer (MCP); the one net (Gaussian)"""
    from .khrylib.rl.core import PolicyGaussian
    from .models.policy_mcp import PolicyMCP
    if isinstance(policy_net, PolicyMCP):
        nets = []
        for net in policy_net.nets:
            a = _act_code(net[0].activation)
            nets.append([(lin, a) for lin in net[0].affine_layers] + [(net[1], ACT_NONE)])
        a = _act_code(policy_net.composer[0].activation)
        nets.append([(lin, a) for lin in policy_net.composer[0].affine_layers])  # (activated after its last layer too, then the softmax)
        return MCP, nets
    if isinstance(policy_net, PolicyGaussian):
        a = _act_code(policy_net.net.activation)
        return GAUSSIAN, [[(lin, a) for lin in policy_net.net.affine_layers] + [(policy_net.action_mean, ACT_NONE)]]
    raise TypeError(f"DevicePolicy.from_modules: PolicyGaussian or PolicyMCP, got {type(policy_net).__name__}")


def _pointer_table(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class DevicePolicy:
    """A frozen policy on the device.  `from_modules` copies the weights and the filter's statistics as they are now; `refresh` copies the weights again
    (a policy that is still being trained, evaluated between epochs).  A handle serves one stream at a time and at most `max_rows` rows per call."""

    def __init__(self, handle, device, modules=None):
        device = torch.device(device)
        if device.index is None:  # ("cuda": the current one, by its number -- tensors report theirs that way)
            device = torch.device(device.type, torch.cuda.current_device())
        self._h, self.device, self._modules = handle, device, modules
        v = [C.c_int32() for _ in range(5)]
        nbytes = C.c_int64()
        check(lib().uhc_policy_dims(handle, *[C.byref(x) for x in v], C.byref(nbytes)))
        self.kind, self.obs_dim, self.act_dim, self.max_rows, self.n_primitives = (int(x.value) for x in v)
        self.packed_bytes = int(nbytes.value)

    # ---- construction
    @classmethod
    def from_modules(cls, policy_net, running_state=None, max_rows=64, device=None):
        kind, nets = _nets_of(policy_net)
        first = nets[0][0][0].weight
        if device is None and first.is_cuda:
            device = first.device
        # (host copies: uhc_policy_create checks them before the first HIP call and uploads them itself)
        arrays = [[(lin.weight.detach().cpu().numpy(), lin.bias.detach().cpu().numpy(), a) for lin, a in net] for net in nets]
        self = cls.from_arrays(kind, first.shape[1], arrays, max_rows=max_rows, device=device)
        self._modules = policy_net
        if running_state is not None:
            self.set_filter(running_state)
        return self

    @classmethod
    def from_arrays(cls, kind, obs_dim, nets, max_rows=64, device=None):
        """nets: per net its layers [(W [out][in], b [out], activation code), ...] as host arrays -- GAUSSIAN: one net; MCP: the primitives, then the composer"""
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        flat = [la for net in nets for la in net]
        w = [np.ascontiguousarray(W, dtype=np.float64) for W, _, _ in flat]
        b = [np.ascontiguousarray(bb, dtype=np.float64) for _, bb, _ in flat]
        for net in nets:  # (the arrays' shapes are what the library will read)
            last = int(obs_dim)
            for W, bb, _ in net:
                if np.ndim(W) != 2 or np.shape(W)[1] != last or np.shape(bb) != (np.shape(W)[0],):
                    raise ValueError(f"DevicePolicy: a layer's weight {np.shape(W)} / bias {np.shape(bb)} does not follow an input of width {last}")
                last = np.shape(W)[0]
        I = C.c_int32
        n_layers = (I * len(nets))(*[len(net) for net in nets])
        widths = (I * len(flat))(*[x.shape[0] for x in w])
        acts = (I * len(flat))(*[int(a) for _, _, a in flat])
        wp = (C.c_void_p * len(flat))(*[x.ctypes.data for x in w])
        bp = (C.c_void_p * len(flat))(*[x.ctypes.data for x in b])
        h = C.c_void_p()
        with torch.cuda.device(device):
            check(lib().uhc_policy_create(int(kind), int(obs_dim), int(w[len(nets[0]) - 1].shape[0]), int(max_rows), len(nets), n_layers, widths, acts, wp, bp, C.byref(h)))
        return cls(h, device)

    def set_filter(self, running_state):
        """the ZFilter's statistics as they are now (n, mean, S) and its demean / destd / clip; None: observations go in as they are"""
        with torch.cuda.device(self.device):
            if running_state is None:
                check(lib().uhc_policy_set_filter(self._h, 0.0, None, None, 0, 0, 0.0))
                return
            rs = running_state.rs
            n = float(rs.n)  # (the property brings the device's statistics to the host first)
            mean, S = np.ascontiguousarray(rs._M, dtype=np.float64), np.ascontiguousarray(rs._S, dtype=np.float64)
            if mean.shape != (self.obs_dim,):
                raise ValueError(f"DevicePolicy.set_filter: the filter's shape {mean.shape} is not ({self.obs_dim},)")
            check(lib().uhc_policy_set_filter(self._h, n, mean.ctypes.data, S.ctypes.data, int(bool(running_state.demean)), int(bool(running_state.destd)),
                                              float(running_state.clip or 0.0)))

    def refresh(self):
        """uhc_policy_set_params from the live modules, on the current stream: device parameters are read where they lie"""
        if self._modules is None:
            raise RuntimeError("DevicePolicy.refresh: this policy was loaded from a file, it has no modules")
        _, nets = _nets_of(self._modules)
        flat = [lin for net in nets for lin, _ in net]
        on_device = flat[0].weight.is_cuda
        w = [lin.weight.detach().to(torch.float64).contiguous() for lin in flat]
        b = [lin.bias.detach().to(torch.float64).contiguous() for lin in flat]
        if on_device and any(t.device != self.device for t in w + b):
            raise ValueError(f"DevicePolicy.refresh: the modules are not on {self.device}")
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            check(lib().uhc_policy_set_params(C.c_void_p(stream.cuda_stream), self._h, _pointer_table(w), _pointer_table(b), int(on_device)))
            if on_device:  # (host arrays: the call has waited for the stream, the copies may go)
                for t in w + b:
                    t.record_stream(stream)

    # ---- the call
    def mean(self, obs, out=None, state_out=None, weight_out=None):
        """obs (n, obs_dim) device float64, rows may be a view into a wider array (stride(1) == 1) -> action means (n, act_dim).  state_out (n, obs_dim):
        the filtered observation; weight_out (n, n_primitives), MCP: the composer's weights."""
        if not (obs.is_cuda and obs.dtype == torch.float64 and obs.dim() == 2 and obs.shape[1] == self.obs_dim and (obs.shape[1] == 1 or obs.stride(1) == 1)):
            raise ValueError(f"DevicePolicy.mean: obs must be a device float64 (n, {self.obs_dim}) tensor with unit column stride")
        if obs.device != self.device:
            raise ValueError(f"DevicePolicy.mean: obs is on {obs.device}, the policy's weights are on {self.device}")
        n = obs.shape[0]
        stride = obs.stride(0) if n > 1 else max(obs.stride(0), self.obs_dim)
        if out is None:
            out = torch.empty((n, self.act_dim), dtype=torch.float64, device=obs.device)
        for t, shape, name in ((out, (n, self.act_dim), "out"), (state_out, (n, self.obs_dim), "state_out"), (weight_out, (n, self.n_primitives), "weight_out")):
            if t is not None and not (t.device == self.device and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape):
                raise ValueError(f"DevicePolicy.mean: {name} must be a contiguous float64 tensor of shape {shape} on {self.device}")
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        check(lib().uhc_policy_act(C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream), self._h, n, p(obs), stride, p(state_out), p(out), p(weight_out)))
        return out

    def select_action(self, x, mean_action=True):
        """what a policy_net's select_action(x, True) returns -- from RAW observations: the filter is inside"""
        if mean_action is not True:
            raise NotImplementedError("DevicePolicy.select_action: mean actions only (sampling: rollout_ops.act on the framework's mean)")
        return self.mean(x)

    # ---- the file
    def save(self, path):
        with torch.cuda.device(self.device):
            check(lib().uhc_policy_save(self._h, str(path).encode()))

    @classmethod
    def load(cls, path, max_rows=64, device=None):
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        h = C.c_void_p()
        with torch.cuda.device(device):
            check(lib().uhc_policy_load(str(path).encode(), int(max_rows), C.byref(h)))
        return cls(h, device)

    def close(self):
        if getattr(self, "_h", None):
            lib().uhc_policy_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
