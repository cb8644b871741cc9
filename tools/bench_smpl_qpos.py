#!/usr/bin/env python3
"""The AMASS -> qpos conversion in front of a device-built clip bank, on the host against on the device (VecHumanoidEnv.set_clip_bank(convert=)), on the
synthetic bank of tools/bench_expert_bank.py (smooth random-walk clips):

  (a) wall time of set_clip_bank(build="device", convert="host"): smpl_to_qpose clip by clip, the qpos rows uploaded, ONE uhc_expert_frames launch;
  (b) wall time of set_clip_bank(build="device", convert="device"): the raw pose / trans arrays uploaded, ONE uhc_smpl_qpos launch, ONE uhc_expert_frames launch;
  (c) smpl_to_qpose on the host alone, clip by clip;
  (d) the kernel's own time from HIP events, as bytes moved -- 576 + 24 read, 608 written per frame -- per second, and beside it a device-to-device copy
      that moves the same number of bytes (read + written), timed in the same process: the yardstick;
  (e) max |host qpos - device qpos| over the bank: faster and different is not faster.

Every figure: warm-up first, a device synchronise inside the timed window, the median of the repeats.  The kernel is timed on the bank tiled up to
--kernel-min-frames frames, so that one launch moves more than the 256 MiB the Infinity Cache holds and lasts long enough to time.

  python tools/bench_smpl_qpos.py [--clips 256] [--frames 300] [--repeats 5] [--out profiles/...txt]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_expert_bank import median_events, median_wall, random_walk_clips  # noqa: E402

READ_B, WRITE_B = (72 + 3) * 8, 76 * 8  # per frame: its pose and translation, its qpos row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5, help="repeats of (a), (b) and (c)")
    ap.add_argument("--kernel-repeats", type=int, default=20)
    ap.add_argument("--kernel-min-frames", type=int, default=537600)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_smpl_qpos: needs the GPU (a time taken elsewhere says nothing about it)")
    from uhc_amd import sim as S
    from uhc_amd._lib import check, lib
    from uhc_amd.envs.humanoid_im import VecHumanoidEnv
    from uhc_amd.smpllib.smpl_mujoco import smpl_to_model_table, smpl_to_qpose
    from uhc_amd.utils.config_utils.copycat_config import Config

    cfg = Config(cfg_id="copycat_mi355x", base_dir=tempfile.mkdtemp(prefix="bench_smpl_qpos_"))
    env = VecHumanoidEnv(cfg, n_env=4)
    clips = random_walk_clips(args.clips, args.frames)
    n_frames = args.clips * args.frames
    sync = torch.cuda.synchronize
    count_offset = cfg.robot_cfg.get("mesh", True)

    def convert():
        return [smpl_to_qpose(pose=c["pose_aa"], mj_model=env.body_model, trans=c["trans"], model="smpl", count_offset=count_offset) for c in clips.values()]

    t_conv, all_conv = median_wall(convert, lambda: None, 1, args.repeats)
    t_host, all_host = median_wall(lambda: env.set_clip_bank(clips, build="device", convert="host"), sync, 1, args.repeats)
    bank_host = env.env._bank[0].clone()
    t_dev, all_dev = median_wall(lambda: env.set_clip_bank(clips, build="device", convert="device"), sync, 1, args.repeats)
    bank_diff = float((bank_host - env.env._bank[0]).abs().max().item())

    # ---- (e) the rows themselves
    pose = np.concatenate([np.asarray(c["pose_aa"], dtype=np.float64).reshape(-1, 72) for c in clips.values()])
    trans = np.concatenate([np.asarray(c["trans"], dtype=np.float64) for c in clips.values()])
    starts = np.arange(0, n_frames, args.frames)
    q_host = np.concatenate(convert())
    q_dev, = S.smpl_qpos_device(pose, trans, starts, env.body_model, count_offset=count_offset)
    max_diff = float(np.abs(q_host - q_dev.cpu().numpy()).max())

    # ---- (d) the kernel alone, on the bank tiled past the Infinity Cache
    reps = max(1, -(-args.kernel_min_frames // n_frames))
    pbig = torch.from_numpy(pose).cuda().repeat(reps, 1).contiguous()
    tbig = torch.from_numpy(trans).cuda().repeat(reps, 1).contiguous()
    nbig = int(pbig.shape[0])
    d_starts = torch.arange(0, nbig, args.frames, dtype=torch.int32, device="cuda")
    off = torch.from_numpy(np.asarray(env.body_model.body_pos, dtype=np.float64)[1:2].copy()).cuda() if count_offset else None
    s2m = np.ascontiguousarray(smpl_to_model_table(env.body_model), dtype=np.int32)
    out = torch.empty((nbig, 76), dtype=torch.float64, device="cuda")
    L = lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def kernel():
        check(L.uhc_smpl_qpos(stream, 24, s2m.ctypes.data_as(C.POINTER(C.c_int32)), None if off is None else C.c_void_p(off.data_ptr()), 1, C.c_void_p(pbig.data_ptr()),
                              C.c_void_p(tbig.data_ptr()), nbig, C.c_void_p(d_starts.data_ptr()), None, int(d_starts.shape[0]), C.c_void_p(out.data_ptr()), None))

    t_k, all_k = median_events(kernel, 3, args.kernel_repeats)
    assert torch.equal(out[:n_frames], q_dev)  # the timed launches computed the bank's rows
    k_bytes = nbig * (READ_B + WRITE_B)
    src = torch.empty(k_bytes // 16, dtype=torch.float64, device="cuda").zero_()  # a copy that moves the same bytes: half of them read, half written
    dst = torch.empty_like(src)
    t_c, all_c = median_events(lambda: dst.copy_(src), 3, args.kernel_repeats)
    c_bytes = 2 * src.numel() * 8
    res = dict(clips=args.clips, frames_per_clip=args.frames, n_frames=n_frames, convert_host_build_s=t_host, convert_device_build_s=t_dev, smpl_to_qpose_host_s=t_conv,
               host_over_device=t_host / t_dev, convert_host_build_all_s=all_host, convert_device_build_all_s=all_dev, smpl_to_qpose_host_all_s=all_conv,
               max_abs_diff_qpos=max_diff, max_abs_diff_bank=bank_diff, kernel_frames=nbig, kernel_s=t_k, kernel_min_s=min(all_k), kernel_max_s=max(all_k),
               kernel_GBps=k_bytes / t_k / 1e9, kernel_Mframes_per_s=nbig / t_k / 1e6, copy_s=t_c, copy_min_s=min(all_c), copy_max_s=max(all_c),
               copy_GBps=c_bytes / t_c / 1e9, kernel_rate_over_copy_rate=(k_bytes / t_k) / (c_bytes / t_c), device=torch.cuda.get_device_name(0))
    lines = [
        f"AMASS -> qpos in front of the clip bank: {args.clips} clips x {args.frames} frames = {n_frames} frames  [{res['device']}]",
        f"(a) set_clip_bank(build='device', convert='host')   {t_host:9.4f} s   (median of {args.repeats}: {', '.join('%.4f' % t for t in all_host)})",
        f"(b) set_clip_bank(build='device', convert='device') {t_dev:9.4f} s   (median of {args.repeats}: {', '.join('%.4f' % t for t in all_dev)})   (a) / (b) = {t_host / t_dev:.2f}",
        f"(c) smpl_to_qpose on the host alone                 {t_conv:9.4f} s   (median of {args.repeats}: {', '.join('%.4f' % t for t in all_conv)})",
        f"(d) uhc_smpl_qpos, {nbig} frames: {t_k * 1e3:.3f} ms (min {min(all_k) * 1e3:.3f}, max {max(all_k) * 1e3:.3f}; median of {args.kernel_repeats}) = "
        f"{res['kernel_GBps']:.1f} GB/s of 600 + 608 B per frame, {res['kernel_Mframes_per_s']:.1f} M frames/s",
        f"    device-to-device copy moving the same {k_bytes / 1e6:.0f} MB: {t_c * 1e3:.3f} ms (min {min(all_c) * 1e3:.3f}, max {max(all_c) * 1e3:.3f}) = "
        f"{res['copy_GBps']:.1f} GB/s read + written;  kernel rate / copy rate = {res['kernel_rate_over_copy_rate']:.3f}",
        f"(e) max |host qpos - device qpos| = {max_diff:.3e};  max |bank (a) - bank (b)| = {bank_diff:.3e}",
    ]
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    env.close()


if __name__ == "__main__":
    main()
