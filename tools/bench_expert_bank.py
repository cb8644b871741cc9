#!/usr/bin/env python3
"""Building the expert clip bank on the host against building it on the device (VecHumanoidEnv.set_clip_bank(build=)), on a synthetic bank
of smooth random-walk clips:

  (a) wall time of set_clip_bank(build="host"): Humanoid.qpos_fk + pack_expert_frames clip by clip, the 4.7 KB records uploaded;
  (b) wall time of set_clip_bank(build="device"): the 608-byte qpos rows uploaded, ONE uhc_expert_frames launch;
      (both contain the AMASS -> qpos conversion on the host, smpl_to_qpose, which is timed on its own beside them)
  (c) the kernel's own time from HIP events, as bytes moved -- 608 read + 4 672 written per frame -- per second, and beside it a
      device-to-device copy of a buffer the size of the bank (read + written bytes per second), timed in the same process: the yardstick.

Every figure: warm-up first, a device synchronise inside the timed window, the median of the repeats.  The kernel is timed on the bank tiled up
to --kernel-min-frames frames, so that one launch moves more than the 256 MiB the Infinity Cache holds and lasts long enough to time.

  python tools/bench_expert_bank.py [--clips 256] [--frames 300] [--repeats 3] [--out profiles/...txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

READ_B, WRITE_B = 76 * 8, 584 * 8  # per frame: its qpos row (the neighbour's comes out of the cache), its record


def random_walk_clips(n_clips, n_frames, seed=3):
    """AMASS-format clips: the shipped standing pose, every axis-angle component on a smoothed random walk (steps of ~0.01 rad per frame)."""
    z = np.load(os.path.join(ROOT, "uhc_amd", "assets", "standing_neutral.npz"))
    base = z["pose_aa"][10].copy()
    rng = np.random.default_rng(seed)
    clips = {}
    for c in range(n_clips):
        steps = rng.normal(scale=0.01, size=(n_frames, 72))
        steps = (steps + np.roll(steps, 1, axis=0) + np.roll(steps, 2, axis=0)) / 3.0
        pose = base[None] + np.cumsum(steps, axis=0)
        trans = np.zeros((n_frames, 3))
        trans[:, :2] = np.cumsum(rng.normal(scale=0.005, size=(n_frames, 2)), axis=0)
        trans[:, 2] = 0.91437225 - 0.0282
        clips[f"walk_{c:05d}"] = dict(pose_aa=pose, trans=trans, beta=np.zeros(16), gender=0)
    return clips


def median_wall(fn, sync, warmup, repeats):
    for _ in range(warmup):
        fn()
        sync()
    ts = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def median_events(fn, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms) * 1e-3, [m * 1e-3 for m in ms]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3, help="repeats of (a) and (b)")
    ap.add_argument("--kernel-repeats", type=int, default=20)
    ap.add_argument("--kernel-min-frames", type=int, default=500000)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_expert_bank: needs the GPU (a time taken elsewhere says nothing about it)")
    from uhc_amd import sim as S
    from uhc_amd._lib import check, lib
    from uhc_amd.envs.humanoid_im import VecHumanoidEnv
    from uhc_amd.smpllib.smpl_mujoco import smpl_to_qpose
    from uhc_amd.utils.config_utils.copycat_config import Config

    cfg = Config(cfg_id="copycat_mi355x", base_dir=tempfile.mkdtemp(prefix="bench_expert_bank_"))
    env = VecHumanoidEnv(cfg, n_env=4)
    clips = random_walk_clips(args.clips, args.frames)
    n_frames = args.clips * args.frames
    sync = torch.cuda.synchronize

    def convert():
        return [smpl_to_qpose(pose=c["pose_aa"], mj_model=env.body_model, trans=c["trans"], model="smpl", count_offset=cfg.robot_cfg.get("mesh", True)) for c in clips.values()]

    t_conv, _ = median_wall(convert, lambda: None, 1, args.repeats)
    t_host, all_host = median_wall(lambda: env.set_clip_bank(clips, build="host"), sync, 1, args.repeats)
    bank_host = env.env._bank[0].clone()
    t_dev, all_dev = median_wall(lambda: env.set_clip_bank(clips, build="device"), sync, 1, args.repeats)
    bank_dev = env.env._bank[0]
    max_diff = float((bank_host - bank_dev).abs().max().item())  # faster and different is not faster

    # ---- (c) the kernel alone, on the bank tiled past the Infinity Cache
    reps = max(1, -(-args.kernel_min_frames // n_frames))
    qpos = torch.from_numpy(np.concatenate(convert())).cuda()
    qbig = qpos.repeat(reps, 1).contiguous()
    nbig = int(qbig.shape[0])
    starts = torch.arange(0, nbig, args.frames, dtype=torch.int32, device="cuda")
    hum = env.humanoid
    off, ioff = hum._offsets[None].cuda().contiguous(), hum._i_offsets[None].cuda().contiguous()
    par, ee = np.ascontiguousarray(hum._parents, dtype=np.int32), np.ascontiguousarray(hum._ee_idx, dtype=np.int32)
    out = torch.empty((nbig, S.FRAME_STRIDE), dtype=torch.float64, device="cuda")
    L = lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def kernel():
        check(L.uhc_expert_frames(stream, 24, par.ctypes.data_as(C.POINTER(C.c_int32)), ee.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(off.data_ptr()),
                                  C.c_void_p(ioff.data_ptr()), 1, C.c_void_p(qbig.data_ptr()), nbig, C.c_void_p(starts.data_ptr()), None, int(starts.shape[0]), None,
                                  1 / 30, C.c_void_p(out.data_ptr())))

    t_k, all_k = median_events(kernel, 3, args.kernel_repeats)
    assert torch.equal(out[:n_frames], bank_dev)  # the timed launches computed the bank
    dst = torch.empty_like(out)
    t_c, all_c = median_events(lambda: dst.copy_(out), 3, args.kernel_repeats)
    k_bytes, c_bytes = nbig * (READ_B + WRITE_B), 2 * nbig * WRITE_B
    res = dict(clips=args.clips, frames_per_clip=args.frames, n_frames=n_frames, bank_MB=n_frames * WRITE_B / 1e6,
               host_build_s=t_host, device_build_s=t_dev, amass_to_qpos_s=t_conv, host_over_device=t_host / t_dev,
               host_build_all_s=all_host, device_build_all_s=all_dev, max_abs_diff_host_device=max_diff,
               kernel_frames=nbig, kernel_s=t_k, kernel_min_s=min(all_k), kernel_max_s=max(all_k), kernel_TBps=k_bytes / t_k / 1e12,
               kernel_Mframes_per_s=nbig / t_k / 1e6, copy_s=t_c, copy_min_s=min(all_c), copy_max_s=max(all_c), copy_TBps=c_bytes / t_c / 1e12,
               kernel_rate_over_copy_rate=(k_bytes / t_k) / (c_bytes / t_c), device=torch.cuda.get_device_name(0))
    lines = [
        f"expert clip bank: {args.clips} clips x {args.frames} frames = {n_frames} frames, {res['bank_MB']:.1f} MB of records  [{res['device']}]",
        f"(a) set_clip_bank(build='host')   {t_host:9.3f} s   (median of {args.repeats}: {', '.join('%.3f' % t for t in all_host)})",
        f"(b) set_clip_bank(build='device') {t_dev:9.3f} s   (median of {args.repeats}: {', '.join('%.3f' % t for t in all_dev)})   host / device = {t_host / t_dev:.2f}",
        f"    of which AMASS -> qpos on the host (smpl_to_qpose, in both) {t_conv:.3f} s;  max |host bank - device bank| = {max_diff:.3e}",
        f"(c) uhc_expert_frames, {nbig} frames: {t_k * 1e3:.3f} ms (min {min(all_k) * 1e3:.3f}, max {max(all_k) * 1e3:.3f}; median of {args.kernel_repeats}) = "
        f"{res['kernel_TBps']:.3f} TB/s of 608 + 4672 B per frame, {res['kernel_Mframes_per_s']:.1f} M frames/s",
        f"    device-to-device copy of the same {nbig * WRITE_B / 1e6:.0f} MB: {t_c * 1e3:.3f} ms (min {min(all_c) * 1e3:.3f}, max {max(all_c) * 1e3:.3f}) = "
        f"{res['copy_TBps']:.3f} TB/s read + written;  kernel rate / copy rate = {res['kernel_rate_over_copy_rate']:.2f}",
    ]
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    env.close()


if __name__ == "__main__":
    main()
