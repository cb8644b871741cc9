#!/usr/bin/env python3
"""Live targets (uhc_env_live_push: one expert frame record per env and control step, appended on the device) at --envs envs:

  (a) one live_push call appending one row to every env's stream: HIP events around blocks of --block calls, per call;
  (b) the host path it replaces, per control step: Humanoid.qpos_fk on one two-frame window per env, pack_expert_frames, one upload of the records
      (wall time, a device synchronise inside the window) -- without the set_bank and the graph re-capture that would follow it;
  (c) a plain device-to-device copy of --envs records (4 672 B each), timed like (a): the floor of anything that writes them;
  (d) the control step of a tracker -- filter, policy, live_push, env.step (uhc_amd.stream.StreamTracker.step) -- against the same step without the
      push on an env that was ASSIGNED the same frames as a clip of a bank; both in this process, on this device, in alternating blocks.

Every figure: a warm-up block first, then the median of --repeats blocks.  States (a)/(c), (b)/(a) and the share of the control step that (d) - plain takes.

  python tools/bench_live_push.py [--envs 1024] [--out profiles/r10_live_push.txt]
"""
import argparse
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
from bench_expert_bank import median_wall, random_walk_clips  # noqa: E402


def block_events(fn, before, block, repeats):
    """per-call seconds of `fn`: HIP events around `block` calls, after `before()` (not timed); one warm-up block, then the median of `repeats`"""
    import torch
    out = []
    for k in range(repeats + 1):
        before()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(block):
            fn(i)
        b.record()
        b.synchronize()
        if k:
            out.append(a.elapsed_time(b) * 1e-3 / block)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--block", type=int, default=50, help="calls per timed block of (a) and (c)")
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20, help="control steps per timed block of (d)")
    ap.add_argument("--step-repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_live_push: needs the GPU (a time taken elsewhere says nothing about it)")
    from uhc_amd import sim as S
    from uhc_amd.envs.humanoid_im import VecHumanoidEnv
    from uhc_amd.khrylib.rl.core import PolicyGaussian
    from uhc_amd.khrylib.utils.zfilter import ZFilter
    from uhc_amd.smpllib.smpl_mujoco import smpl_to_qpose
    from uhc_amd.stream import StreamTracker
    from uhc_amd.utils.config_utils.copycat_config import Config

    n, T = args.envs, args.block + 2
    cfg = Config(cfg_id="copycat_mi355x", base_dir=tempfile.mkdtemp(prefix="bench_live_push_"))
    cfg.env_init_noise = 0.0
    live = VecHumanoidEnv(cfg, n_env=n, mode="test")
    clips = random_walk_clips(1, max(T, args.steps + 4))
    (key, clip), = clips.items()
    rows_h = np.asarray(smpl_to_qpose(pose=clip["pose_aa"], mj_model=live.body_model, trans=clip["trans"], model="smpl", count_offset=cfg.robot_cfg.get("mesh", True)), dtype=np.float64)
    rows = [torch.from_numpy(np.tile(r, (n, 1))).cuda() for r in rows_h]  # frame t of every env (the same motion in all of them)
    ids = torch.arange(n, dtype=torch.int32, device="cuda")
    ones = torch.ones(n, dtype=torch.int32, device="cuda")
    sync = torch.cuda.synchronize

    # ---- (a) one live_push call
    live.live_begin(T)
    t_push, all_push = block_events(lambda i: live.env.live_push(ids, rows[i + 1]), lambda: live.env.live_push(ids, rows[0], restart=ones), args.block, args.repeats)
    assert live.live_view()[1].cpu().tolist() == [args.block + 1] * n and int(live.live_view()[2].sum()) == 0  # every timed call appended

    # ---- (c) a plain copy of n records
    src = torch.zeros((n, S.FRAME_STRIDE), dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    t_copy, all_copy = block_events(lambda i: dst.copy_(src), lambda: None, args.block, args.repeats)

    # ---- (b) the host path per control step: n two-frame windows through qpos_fk, packed, uploaded
    hum = live.humanoid
    win = torch.from_numpy(rows_h[:2].copy())

    def host_path():
        recs = np.stack([S.pack_expert_frames(hum.qpos_fk(win.clone()))[1] for _ in range(n)])
        return torch.from_numpy(recs).cuda()

    t_host, all_host = median_wall(host_path, sync, 1, args.host_repeats)

    # ---- (d) the control step with and without the push
    bank = VecHumanoidEnv(cfg, n_env=n, mode="test")
    bank.set_clip_bank(clips, build="device")
    torch.manual_seed(0)
    pol = PolicyGaussian(types.SimpleNamespace(policy_hsize=list(cfg.policy_hsize), policy_htype=cfg.policy_htype, fix_std=True, log_std=-2.3),
                         action_dim=live.action_dim, state_dim=live.obs_dim).double().cuda()
    filt = ZFilter((live.obs_dim,), clip=5)
    filt.set_mean_std(np.zeros(live.obs_dim), np.full(live.obs_dim, 9.0), 10)
    tracker = StreamTracker(live, pol, filt)
    head = torch.stack(rows[:3], 1)
    keys = [key] * n

    def plain_block():
        bank.assign(np.arange(n), keys, np.zeros(n, dtype=int), np.full(n, args.steps + 4))
        bank.reset(np.arange(n))
        sync()
        t0 = time.perf_counter()
        with torch.no_grad():
            for t in range(args.steps):
                bank.step(pol.select_action(filt(bank.obs.to(torch.float64), update=False), True).to(torch.float64).contiguous())
        sync()
        return (time.perf_counter() - t0) / args.steps

    def live_block():
        live.live_begin(args.steps + 4)
        tracker.begin(head)
        sync()
        t0 = time.perf_counter()
        for t in range(args.steps):
            tracker.step(rows[t + 3])
        sync()
        return (time.perf_counter() - t0) / args.steps

    plain, tracked = [], []
    for k in range(args.step_repeats + 1):  # alternating blocks; the first pair warms up
        p, q = plain_block(), live_block()
        if k:
            plain.append(p)
            tracked.append(q)
    same = bool(torch.equal(live.sim.field(S.F_QPOS), bank.sim.field(S.F_QPOS)))  # the two envs computed the same trajectory
    t_plain, t_track = statistics.median(plain), statistics.median(tracked)

    res = dict(envs=n, live_push_s=t_push, live_push_all_s=all_push, copy_s=t_copy, copy_all_s=all_copy, host_path_s=t_host, host_path_all_s=all_host,
               push_over_copy=t_push / t_copy, host_over_push=t_host / t_push, plain_step_s=t_plain, plain_step_all_s=plain, tracker_step_s=t_track,
               tracker_step_all_s=tracked, push_share_of_step=(t_track - t_plain) / t_track, same_trajectory=same, device=torch.cuda.get_device_name(0))
    us = lambda ts: ", ".join("%.1f" % (t * 1e6) for t in ts)  # noqa: E731
    lines = [
        f"live targets at {n} envs  [{res['device']}]",
        f"(a) one live_push call, {n} rows appended:      {t_push * 1e6:9.1f} us  (HIP events, blocks of {args.block} calls; median of {args.repeats}: {us(all_push)})",
        f"(b) host path: {n} x qpos_fk(2 frames), pack, upload: {t_host * 1e3:9.1f} ms  (wall; median of {args.host_repeats}: {', '.join('%.1f' % (t * 1e3) for t in all_host)})",
        f"(c) device copy of {n} records ({n * 4672 / 1e6:.2f} MB):      {t_copy * 1e6:9.1f} us  (HIP events, blocks of {args.block}; median of {args.repeats}: {us(all_copy)})",
        f"    (a) / (c) = {t_push / t_copy:.2f};  (b) / (a) = {t_host / t_push:.0f}",
        f"(d) control step, filter + policy + env.step, bank-assigned clip: {t_plain * 1e3:.3f} ms  (wall, blocks of {args.steps} steps; median of {args.step_repeats}: {', '.join('%.3f' % (t * 1e3) for t in plain)})",
        f"    StreamTracker.step (the same + live_push), live stream:      {t_track * 1e3:.3f} ms  ({', '.join('%.3f' % (t * 1e3) for t in tracked)})",
        f"    difference {1e6 * (t_track - t_plain):.1f} us = {100 * res['push_share_of_step']:.2f} % of the tracker's control step;  same trajectory in both envs: {same}",
    ]
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    live.close()
    bank.close()


if __name__ == "__main__":
    main()
