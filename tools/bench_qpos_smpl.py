#!/usr/bin/env python3
"""Handing a tracked motion back as SMPL parameters (axis-angle pose + translation), on the device against on the host:

  (a) wall time of StreamTracker.step at --envs envs (live mode, a random frozen policy) without and with smpl=True -- the same run, the two kinds of step
      alternating, so that both see the same drift of the motion; the increment is what uhc_qpos_smpl costs a control step.  Where it drowns in the step's
      own spread, env.smpl_pose() alone, back to back from HIP events, says what a call costs;
  (b) the host route for the same state: the blocking readback of the qpos field + qpos_to_smpl (a Python loop over 23 joints of scipy calls);
  (c) the kernel's own time from HIP events on --kernel-rows hinge rows (608 B read, 576 + 24 B written per row), as bytes per second, and beside it a
      device-to-device copy that moves the same number of bytes (read + written), timed in the same process: the yardstick;
  (d) max |host - device| of pose and translation on (a)'s last state: faster and different is not faster.

Every figure: warm-up first, a device synchronise inside the timed window, the median of the repeats.

  python tools/bench_qpos_smpl.py [--envs 1024] [--steps 200] [--kernel-rows 1048576] [--out profiles/...txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_expert_bank import median_events, median_wall, random_walk_clips  # noqa: E402

READ_B, WRITE_B = 76 * 8, (72 + 3) * 8  # per row: its qpos row, its pose and translation


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200, help="timed control steps of (a): half of them with smpl=True")
    ap.add_argument("--repeats", type=int, default=5, help="repeats of (b)")
    ap.add_argument("--kernel-repeats", type=int, default=20)
    ap.add_argument("--kernel-rows", type=int, default=1 << 20)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_qpos_smpl: needs the GPU (a time taken elsewhere says nothing about it)")
    from uhc_amd import sim as S
    from uhc_amd._lib import check, lib
    from uhc_amd.envs.humanoid_im import VecHumanoidEnv
    from uhc_amd.khrylib.rl.core import PolicyGaussian
    from uhc_amd.smpllib.smpl_mujoco import qpos_to_smpl, smpl_to_model_table
    from uhc_amd.stream import StreamTracker
    from uhc_amd.utils.config_utils.copycat_config import Config

    n, warm = args.envs, 6
    cfg = Config(cfg_id="copycat_mi355x", base_dir=tempfile.mkdtemp(prefix="bench_qpos_smpl_"))
    cfg.env_init_noise = 0.0
    env = VecHumanoidEnv(cfg, n_env=n, mode="test")
    sync = torch.cuda.synchronize
    T = 3 + warm + args.steps
    clips = random_walk_clips(8, T)
    pose = np.stack([clips[k]["pose_aa"] for k in clips])[np.arange(n) % 8]   # [env][frame][72]
    trans = np.stack([clips[k]["trans"] for k in clips])[np.arange(n) % 8]
    (rows,) = S.smpl_qpos_device(pose.reshape(n * T, 72), trans.reshape(n * T, 3), np.arange(0, n * T, T), env.body_model, count_offset=cfg.robot_cfg.get("mesh", True))
    rows = rows.view(n, T, 76)
    torch.manual_seed(3)
    pol = PolicyGaussian(types.SimpleNamespace(policy_hsize=[1024, 512], policy_htype="gelu", fix_std=True, log_std=-2.3), action_dim=env.action_dim,
                         state_dim=env.obs_dim).double().cuda()
    env.live_begin(T)
    tr = StreamTracker(env, pol, None)
    tr.begin(rows[:, :3].contiguous())
    for t in range(warm):
        tr.step(rows[:, 3 + t].contiguous(), smpl=bool(t & 1))
    sync()
    plain, with_smpl = [], []
    for t in range(args.steps):
        nxt = rows[:, 3 + warm + t].contiguous()
        sync()
        t0 = time.perf_counter()
        tr.step(nxt, smpl=bool(t & 1))
        sync()
        (with_smpl if t & 1 else plain).append(time.perf_counter() - t0)
    t_plain, t_smpl = statistics.median(plain), statistics.median(with_smpl)

    # ---- (b) the host route on the same state, and (d) what the two routes give
    qf = env.sim.field(S.F_QPOS)

    def host_route():
        return qpos_to_smpl(qf.cpu().numpy(), env.body_model)

    t_host, all_host = median_wall(host_route, lambda: None, 1, args.repeats)
    t_read, all_read = median_wall(lambda: qf.cpu().numpy(), lambda: None, 1, args.repeats)
    h_pose, h_trans = host_route()
    d_pose, d_trans = env.smpl_pose()
    diff_pose = float(np.abs(d_pose.cpu().numpy() - h_pose.reshape(n, 72)).max())
    diff_trans = float(np.abs(d_trans.cpu().numpy() - h_trans).max())

    # ---- (a') what the step gains: env.smpl_pose() alone, HIP events over runs of 50 launches
    def fifty():
        for _ in range(50):
            env.smpl_pose()

    t_50, all_50 = median_events(fifty, 2, 10)
    t_launch = t_50 / 50

    # ---- (c) the kernel alone, on rows tiled past the Infinity Cache
    nbig = args.kernel_rows
    big = qf[:, :76].repeat(-(-nbig // n), 1)[:nbig].contiguous()
    out_p = torch.empty((nbig, 72), dtype=torch.float64, device="cuda")
    out_t = torch.empty((nbig, 3), dtype=torch.float64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    off = torch.from_numpy(np.asarray(env.body_model.body_pos, dtype=np.float64)[1:2].copy()).cuda()
    s2m = np.ascontiguousarray(smpl_to_model_table(env.body_model), dtype=np.int32)
    L = lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def kernel():
        check(L.uhc_qpos_smpl(stream, 24, s2m.ctypes.data_as(C.POINTER(C.c_int32)), 0, p(off), 1, p(big), 76, nbig, 1, None, None, p(out_p), p(out_t), None, p(bad), None))

    t_k, all_k = median_events(kernel, 3, args.kernel_repeats)
    # the timed launches computed (a)'s poses
    assert np.array_equal(out_p[:n].cpu().numpy(), d_pose.cpu().numpy(), equal_nan=True) and np.array_equal(out_t[:n].cpu().numpy(), d_trans.cpu().numpy(), equal_nan=True)
    assert int(bad.item()) == 0, f"{int(bad.item())} of the {nbig} rows hold a state the simulation has lost"
    k_bytes = nbig * (READ_B + WRITE_B)
    src = torch.empty(k_bytes // 16, dtype=torch.float64, device="cuda").zero_()  # a copy that moves the same bytes: half of them read, half written
    dst = torch.empty_like(src)
    t_c, all_c = median_events(lambda: dst.copy_(src), 3, args.kernel_repeats)
    c_bytes = 2 * src.numel() * 8
    res = dict(envs=n, steps=args.steps, step_s=t_plain, step_smpl_s=t_smpl, step_increment_s=t_smpl - t_plain, smpl_pose_launch_s=t_launch, smpl_pose_launch_min_s=min(all_50) / 50, smpl_pose_launch_max_s=max(all_50) / 50, step_all_s=plain, step_smpl_all_s=with_smpl,
               host_route_s=t_host, host_route_all_s=all_host, readback_s=t_read, readback_all_s=all_read, host_over_smpl_pose_launch=t_host / t_launch,
               max_abs_diff_pose=diff_pose, max_abs_diff_trans=diff_trans, kernel_rows=nbig, kernel_s=t_k, kernel_min_s=min(all_k), kernel_max_s=max(all_k),
               kernel_GBps=k_bytes / t_k / 1e9, kernel_Mrows_per_s=nbig / t_k / 1e6, copy_s=t_c, copy_min_s=min(all_c), copy_max_s=max(all_c),
               copy_GBps=c_bytes / t_c / 1e9, kernel_rate_over_copy_rate=(k_bytes / t_k) / (c_bytes / t_c), device=torch.cuda.get_device_name(0))
    lines = [
        f"qpos -> SMPL pose + translation behind a control step: {n} envs, {args.steps} timed steps  [{res['device']}]",
        f"(a) StreamTracker.step()          {t_plain * 1e3:9.3f} ms   (median of {len(plain)}: min {min(plain) * 1e3:.3f}, max {max(plain) * 1e3:.3f})",
        f"    StreamTracker.step(smpl=True) {t_smpl * 1e3:9.3f} ms   (median of {len(with_smpl)}: min {min(with_smpl) * 1e3:.3f}, max {max(with_smpl) * 1e3:.3f})   "
        f"increment {(t_smpl - t_plain) * 1e3:+.3f} ms",
        f"    env.smpl_pose() alone, back to back: {t_launch * 1e6:.1f} us a call (HIP events over runs of 50; min {min(all_50) / 50 * 1e6:.1f}, max {max(all_50) / 50 * 1e6:.1f})",
        f"(b) host route: readback + qpos_to_smpl {t_host * 1e3:9.3f} ms   (median of {args.repeats}: {', '.join('%.3f' % (t * 1e3) for t in all_host)});  "
        f"the readback alone {t_read * 1e3:.3f} ms",
        f"(c) uhc_qpos_smpl, {nbig} rows: {t_k * 1e3:.3f} ms (min {min(all_k) * 1e3:.3f}, max {max(all_k) * 1e3:.3f}; median of {args.kernel_repeats}) = "
        f"{res['kernel_GBps']:.1f} GB/s of 608 + 600 B per row, {res['kernel_Mrows_per_s']:.1f} M rows/s",
        f"    device-to-device copy moving the same {k_bytes / 1e6:.0f} MB: {t_c * 1e3:.3f} ms (min {min(all_c) * 1e3:.3f}, max {max(all_c) * 1e3:.3f}) = "
        f"{res['copy_GBps']:.1f} GB/s read + written;  kernel rate / copy rate = {res['kernel_rate_over_copy_rate']:.3f}",
        f"(d) max |host pose_aa - device pose_aa| = {diff_pose:.3e};  max |host trans - device trans| = {diff_trans:.3e}",
    ]
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    env.close()


if __name__ == "__main__":
    main()
