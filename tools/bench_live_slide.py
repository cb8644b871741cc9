#!/usr/bin/env python3
"""Endless live streams (uhc_env_live_slide: a push to a full stream first moves the records the env can still read to the front of its slice) at --envs envs,
one process, one device:

  (a) one live_push call appending one row to every env's stream, HIP events around blocks of --block calls, per call, in three variants that alternate
      within the run: sliding OFF on a bank that holds the whole block (the reference point), sliding ON at cap 16, sliding ON at cap 4 (every push slides).
      The consumer is played by `cur_t += 1` on the env's own counter after every push -- in all three variants, so the difference is the slide's --;
      beside each, records moved per pushed row (the live_window counter);
  (b) the control step of a tracker (uhc_amd.stream.StreamTracker.step: filter, policy, live_push, env.step) on a sliding bank of cap 16 against a
      non-sliding bank that holds the whole run, over the same frames, in alternating blocks of --steps steps (wall time per step); the final states of the
      two are asserted equal;
  (c) the bytes of the two banks.

Every figure: a warm-up block first, then the median of the repeats.

  python tools/bench_live_slide.py [--envs 1024] [--out profiles/r13_live_slide.txt]
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
from bench_expert_bank import random_walk_clips  # noqa: E402

HEAD = 3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--block", type=int, default=50, help="calls per timed block of (a)")
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--steps", type=int, default=60, help="control steps per timed block of (b)")
    ap.add_argument("--step-repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_live_slide: needs the GPU (a time taken elsewhere says nothing about it)")
    from uhc_amd import sim as S
    from uhc_amd.envs.humanoid_im import VecHumanoidEnv
    from uhc_amd.khrylib.rl.core import PolicyGaussian
    from uhc_amd.khrylib.utils.zfilter import ZFilter
    from uhc_amd.smpllib.smpl_mujoco import smpl_to_qpose
    from uhc_amd.stream import StreamTracker
    from uhc_amd.utils.config_utils.copycat_config import Config

    n = args.envs
    n_rows = max(args.block, args.steps) + HEAD + 1
    cfg = Config(cfg_id="copycat_mi355x", base_dir=tempfile.mkdtemp(prefix="bench_live_slide_"))
    cfg.env_init_noise = 0.0
    wide, slid = VecHumanoidEnv(cfg, n_env=n, mode="test"), VecHumanoidEnv(cfg, n_env=n, mode="test")
    (key, clip), = random_walk_clips(1, n_rows).items()
    rows_h = np.asarray(smpl_to_qpose(pose=clip["pose_aa"], mj_model=wide.body_model, trans=clip["trans"], model="smpl", count_offset=cfg.robot_cfg.get("mesh", True)), dtype=np.float64)
    rows = [torch.from_numpy(np.tile(r, (n, 1))).cuda() for r in rows_h]  # frame t of every env (the same motion in all of them)
    ids = torch.arange(n, dtype=torch.int32, device="cuda")
    ones = torch.ones(n, dtype=torch.int32, device="cuda")
    sync = torch.cuda.synchronize

    # ---- (a) one live_push call, three variants in alternating blocks
    variants = [("off", args.block + HEAD + 1, False), ("on16", 16, True), ("on4", 4, True)]
    cur_t = slid.env.field(S.E_CUR_T)
    times = {v[0]: [] for v in variants}
    moved = {}
    for k in range(args.repeats + 1):  # the first round warms up
        for name, cap, slide in variants:
            slid.live_begin(cap, slide=slide)
            for t in range(HEAD):
                slid.env.live_push(ids, rows[t], restart=ones if t == 0 else None)
            slid.reset(np.arange(n))
            sync()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(args.block):
                slid.env.live_push(ids, rows[i + HEAD])
                cur_t.add_(1)
            b.record()
            b.synchronize()
            _, ln, dr = slid.live_view()
            base, mv = slid.live_window()
            assert int(dr.sum()) == 0 and (base + ln).cpu().tolist() == [args.block + HEAD] * n, name  # every timed call appended
            moved[name] = float(mv.sum()) / (n * args.block)
            if k:
                times[name].append(a.elapsed_time(b) * 1e-3 / args.block)
    t_a = {name: statistics.median(ts) for name, ts in times.items()}

    # ---- (b) the tracker's control step on a sliding bank of 16 frames and on a bank that holds the run
    torch.manual_seed(0)
    pol = PolicyGaussian(types.SimpleNamespace(policy_hsize=list(cfg.policy_hsize), policy_htype=cfg.policy_htype, fix_std=True, log_std=-2.3),
                         action_dim=wide.action_dim, state_dim=wide.obs_dim).double().cuda()
    filt = ZFilter((wide.obs_dim,), clip=5)
    filt.set_mean_std(np.zeros(wide.obs_dim), np.full(wide.obs_dim, 9.0), 10)
    head = torch.stack(rows[:HEAD], 1)
    cap_wide = args.steps + HEAD + 1
    trackers = {"wide": StreamTracker(wide, pol, filt), "slid": StreamTracker(slid, pol, filt)}

    def block(which):
        env = wide if which == "wide" else slid
        env.live_begin(cap_wide if which == "wide" else 16, slide=which == "slid")
        trackers[which].begin(head)
        sync()
        t0 = time.perf_counter()
        for t in range(args.steps):
            trackers[which].step(rows[t + HEAD])
        sync()
        return (time.perf_counter() - t0) / args.steps

    steps = {"wide": [], "slid": []}
    for k in range(args.step_repeats + 1):  # alternating blocks; the first pair warms up
        for which in ("wide", "slid"):
            t = block(which)
            if k:
                steps[which].append(t)
    same = bool(torch.equal(wide.sim.field(S.F_QPOS), slid.sim.field(S.F_QPOS)) and torch.equal(wide.sim.field(S.F_QVEL), slid.sim.field(S.F_QVEL))
                and torch.equal(wide.obs, slid.obs) and torch.equal(wide.done, slid.done))
    assert same, "the sliding env and the unbounded env must end in the same state"
    assert int(slid.live_view()[2].sum()) == 0 and int(wide.live_view()[2].sum()) == 0
    moved_b = float(slid.live_window()[1].sum()) / (n * args.steps)
    t_wide, t_slid = statistics.median(steps["wide"]), statistics.median(steps["slid"])

    # ---- (c) the banks
    bytes_wide, bytes_slid = n * cap_wide * 4672, n * 16 * 4672

    res = dict(envs=n, block=args.block, push_off_s=t_a["off"], push_on16_s=t_a["on16"], push_on4_s=t_a["on4"], push_all_s=times, moved_per_push=moved,
               step_wide_s=t_wide, step_slid_s=t_slid, step_all_s=steps, moved_per_push_tracker=moved_b, slide_share_of_step=(t_slid - t_wide) / t_slid,
               same_final_state=same, bank_bytes_wide=bytes_wide, bank_bytes_slid=bytes_slid, steps=args.steps, device=torch.cuda.get_device_name(0))
    us = lambda ts: ", ".join("%.1f" % (t * 1e6) for t in ts)  # noqa: E731
    ms = lambda ts: ", ".join("%.3f" % (t * 1e3) for t in ts)  # noqa: E731
    lines = [
        f"endless live streams at {n} envs  [{res['device']}]",
        f"(a) one live_push call of {n} rows + cur_t += 1 (HIP events, blocks of {args.block} calls, the variants alternating; median of {args.repeats})",
        f"    sliding off, cap {args.block + HEAD + 1}: {t_a['off'] * 1e6:8.1f} us   moved / push {moved['off']:.3f}   ({us(times['off'])})",
        f"    sliding on,  cap 16: {t_a['on16'] * 1e6:8.1f} us   moved / push {moved['on16']:.3f}   ({us(times['on16'])})   + {(t_a['on16'] - t_a['off']) * 1e6:.1f} us",
        f"    sliding on,  cap  4: {t_a['on4'] * 1e6:8.1f} us   moved / push {moved['on4']:.3f}   ({us(times['on4'])})   + {(t_a['on4'] - t_a['off']) * 1e6:.1f} us",
        f"(b) StreamTracker.step, wall per step, alternating blocks of {args.steps} steps; median of {args.step_repeats}",
        f"    non-sliding bank of cap {cap_wide}: {t_wide * 1e3:.3f} ms  ({ms(steps['wide'])})",
        f"    sliding bank of cap 16:      {t_slid * 1e3:.3f} ms  ({ms(steps['slid'])})   moved / push {moved_b:.3f}",
        f"    difference {(t_slid - t_wide) * 1e6:.1f} us = {100 * res['slide_share_of_step']:.2f} % of the control step;  same final state: {same}",
        f"(c) bank: {bytes_wide / 1e6:.1f} MB for the {args.steps}-step run without sliding (it grows with the run), {bytes_slid / 1e6:.1f} MB with cap 16 (it does not)",
    ]
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    wide.close()
    slid.close()


if __name__ == "__main__":
    main()
