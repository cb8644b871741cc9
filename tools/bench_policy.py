#!/usr/bin/env python
"""Time per call of the mean action, raw observations -> action tensor, on the two release architectures and 1 .. 4096 rows:

  (a)  uhc_policy_act (uhc_amd.policy_ops.DevicePolicy.mean: filter fused, one launch per layer), eager
  (a') the same call captured in a HIP graph
  (b)  today's path, eager: ZFilter(update=False) + policy_net.select_action(state, True) + .contiguous()
  (c)  (b) captured in a HIP graph
  (d)  a plain device copy of as many bytes as the packed weights and biases hold: the floor of a call that reads every weight once

Every figure is the median over BLOCKS timed blocks of REPS back-to-back calls (wall clock, the device synchronised at both ends of a block) behind a warm-up.
Nothing is asserted: the table is the result, including the shapes where the framework wins.

Below the table the tool writes the accuracy figures of the same cases tests/test_gpu_policy.py asserts on: per case d_fw (torch's own device forward against
torch CPU on the same inputs), the kernel's error against torch CPU, and the tolerance max(4 d_fw, 1e-14) the tests grant.  The whole of
profiles/r15_policy_act.txt (--out) is this tool's output: running it again rewrites every section."""
import argparse
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROWS = (1, 16, 64, 1024, 4096)
OBS, ACT = 643, 69


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def _policies():
    from uhc_amd.khrylib.rl.core import PolicyGaussian
    from uhc_amd.models.policy_mcp import PolicyMCP
    torch.manual_seed(0)
    yield "Gaussian gelu 643 -> 2048 -> 1024 -> 512 -> 69", PolicyGaussian(types.SimpleNamespace(policy_hsize=[2048, 1024, 512], policy_htype="gelu", fix_std=True, log_std=-2.3),
                                                                          action_dim=ACT, state_dim=OBS).double().cuda()
    yield "MCP relu 8 x (643 -> 512 -> 256 -> 69), composer 643 -> 300 -> 200 -> 8", PolicyMCP(
        _Cfg(policy_hsize=[512, 256], policy_htype="relu", fix_std=True, log_std=-2.3, num_primitive=8, composer_dim=[300, 200]), action_dim=ACT, state_dim=OBS).double().cuda()


def _time(fn, reps, blocks, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        per_call.append((time.perf_counter() - t0) / reps)
    return statistics.median(per_call) * 1e6, min(per_call) * 1e6, max(per_call) * 1e6


def _graph(fn):
    import gc
    fn()
    torch.cuda.synchronize()
    gc.collect()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def _identity(x):
    return x


def _accuracy():
    """-> lines: d_fw and the kernel's own error per case, reference torch CPU float64 (the cases of tests/test_gpu_policy.py, the same seeds)"""
    import copy
    from uhc_amd import policy_ops as PO
    from uhc_amd.khrylib.rl.core import PolicyGaussian
    from uhc_amd.models.policy_mcp import PolicyMCP

    def figures(pol, dp, x, what):
        with torch.no_grad():
            ref = pol(x).loc
            fw = copy.deepcopy(pol).cuda()(x.cuda()).loc.cpu()
        got = dp.mean(x.cuda()).cpu()
        d_fw, err = float((fw - ref).abs().max()), float((got - ref).abs().max())
        return f"{what}: d_fw = {d_fw:.3e}  kernel error = {err:.3e}  tolerance = {max(4.0 * d_fw, 1e-14):.3e}  max |mean| = {float(ref.abs().max()):.3e}"

    def gaussian(state_dim, hsize, action_dim, htype, seed):
        torch.manual_seed(seed)
        pol = PolicyGaussian(types.SimpleNamespace(policy_hsize=list(hsize), policy_htype="tanh" if htype == "none" else htype, fix_std=True, log_std=-2.3),
                             action_dim=action_dim, state_dim=state_dim).double()
        pol.action_mean.bias.data.normal_(std=0.1)
        if htype != "none":
            return pol, lambda rows: PO.DevicePolicy.from_modules(pol, max_rows=rows)
        pol.net.activation = _identity
        layers = [(l.weight.detach().numpy(), l.bias.detach().numpy(), PO.ACT_NONE) for l in list(pol.net.affine_layers) + [pol.action_mean]]
        return pol, lambda rows: PO.DevicePolicy.from_arrays(PO.GAUSSIAN, state_dim, [layers], max_rows=rows)

    lines = ["Accuracy.  Reference: the torch modules in float64 on the CPU.  d_fw = torch's own device forward against torch CPU on the same inputs;",
             "tolerance = max(4 d_fw, 1e-14), what tests/test_gpu_policy.py grants the kernel; max |mean| = the size of the values compared.", ""]
    g = np.load(os.path.join(ROOT, "tests", "golden", "g12_policy_mcp.npz"))
    pol = PolicyMCP(_Cfg(policy_hsize=[24, 16, 12], policy_htype="gelu", fix_std=True, log_std=-2.3, num_primitive=4, composer_dim=[20, 10]), action_dim=7, state_dim=19).double()
    pol.load_state_dict({k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("pol_")})
    x = torch.from_numpy(g["x"])
    dp = PO.DevicePolicy.from_modules(pol, max_rows=32)
    lines.append(figures(pol, dp, x, "g12 MCP 19 -> 24 -> 16 -> 12 -> 7 x 4, composer 19 -> 20 -> 10 -> 4, 32 rows"))
    w = torch.empty(32, 4, dtype=torch.float64, device="cuda")
    dp.mean(x.cuda(), weight_out=w)
    with torch.no_grad():
        wref = pol.composer(x)
        wfw = copy.deepcopy(pol).cuda().composer(x.cuda()).cpu()
    lines.append(f"g12 composer weight: d_fw = {float((wfw - wref).abs().max()):.3e}  kernel error = {float((w.cpu() - wref).abs().max()):.3e}  "
                 f"against the golden: mean {np.abs(dp.mean(x.cuda()).cpu().numpy() - g['mean']).max():.3e}  weight {np.abs(w.cpu().numpy() - g['weight']).max():.3e}")
    dp.close()
    for i, htype in enumerate(("none", "tanh", "relu", "sigmoid", "gelu")):
        pol, make = gaussian(5, [17, 33], 3, htype, i)
        dp = make(65)
        torch.manual_seed(11)
        X = torch.randn(65, 5, dtype=torch.float64) * 2.0
        for rows in (1, 15, 16, 17, 65):
            lines.append(figures(pol, dp, X[:rows], f"Gaussian 5 -> 17 -> 33 -> 3 {htype}, {rows} rows"))
        dp.close()
    pol, make = gaussian(643, [2048, 1024, 512], 69, "gelu", 5)
    dp = make(48)
    torch.manual_seed(12)
    lines.append(figures(pol, dp, torch.randn(48, 643, dtype=torch.float64), "Gaussian 643 -> 2048 -> 1024 -> 512 -> 69 gelu, 48 rows"))
    dp.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_policy_act.txt"))
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    from uhc_amd.khrylib.utils.zfilter import ZFilter
    from uhc_amd.policy_ops import DevicePolicy
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?")
    lines = [f"tools/bench_policy.py on {torch.cuda.get_device_name(0)} ({arch}; the name is what the runtime reports for the card, the architecture tells the MI355X: gfx950): microseconds per call, median (min .. max) of {args.blocks} blocks of {args.reps} calls, "
             f"warm-up {args.warmup} calls; float64", ""]
    rng = np.random.default_rng(0)
    filt = ZFilter((OBS,), clip=5)
    filt.set_mean_std(rng.normal(scale=0.1, size=OBS), rng.uniform(0.5, 2.0, size=OBS) * 9, 10)
    for name, pol in _policies():
        lines += [name, f"{'rows':>6} {'(a) uhc_policy_act':>26} {'(a) in a graph':>26} {'(b) torch eager':>26} {'(c) torch in a graph':>26} {'(d) copy of the weights':>26}   (b)/(a)  (c)/(a')"]
        for rows in ROWS:
            reps = args.reps if rows <= 1024 else max(args.reps // 5, 5)
            dp = DevicePolicy.from_modules(pol, filt, max_rows=rows)
            obs = torch.randn(rows, OBS, dtype=torch.float64, device="cuda")
            out = torch.empty(rows, ACT, dtype=torch.float64, device="cuda")
            src = torch.empty(dp.packed_bytes, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            box = {}

            def device():
                dp.mean(obs, out=out)

            def eager():
                with torch.no_grad():
                    box["a"] = pol.select_action(filt(obs, update=False), True).to(torch.float64).contiguous()

            def copy():
                dst.copy_(src)

            res = [_time(f, reps, args.blocks, args.warmup) for f in (device, _graph(device), eager, _graph(eager), copy)]
            cells = " ".join(f"{m:10.1f} ({lo:6.1f}..{hi:6.1f})" for m, lo, hi in res)
            lines.append(f"{rows:>6} {cells}   {res[2][0] / res[0][0]:7.2f}  {res[3][0] / res[1][0]:7.2f}")
            print(lines[-1], flush=True)
            dp.close()
        lines.append(f"  packed weights and biases: {dp.packed_bytes} bytes")
        lines.append("")
    lines += _accuracy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
