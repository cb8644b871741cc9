#!/usr/bin/env python3
"""What the surface metrics (config key eval_surface: penetration, skate, float, contact count on the hull vertices) cost, on one MI355X, synthetic clips:

  (a) wall time of AgentCopycat.eval_seqs with eval_build "device", eval_surface off against on: what the feature adds to an evaluation pass
      (uhc_eval_record_pose before every uhc_eval_record, one uhc_surface_metrics launch, three more words per clip and one per row in the chunk's copy);
  (b) uhc_surface_metrics alone (HIP events) on a pose record of the pass's shape -- the expert poses of the clips, in the record's layout --
      against the host functions on the same record (the device -> host copy of the poses included: hull_vertices, compute_penetration, compute_skate,
      compute_float, compute_contact clip by clip), and against a plain device copy of the bytes the launch reads;
  (c) uhc_eval_record_pose alone (HIP events over a run of launches) beside the time of a control step of the pass (a).

Every figure: a warm-up first, a device synchronise inside the timed window, the median of the repeats; the running filter's state is put back before
every pass, so that all passes run the same episodes; off and on alternate.

  python tools/bench_surface.py [--clips 256] [--frames 300] [--n-env 256] [--repeats 3] [--out profiles/...txt]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--frames", type=int, default=300, help="clip lengths are drawn from [frames - 20, frames + 20]")
    ap.add_argument("--n-env", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface: needs the GPU (a time taken elsewhere says nothing about it)")
    from uhc_amd import eval_ops as EO
    from uhc_amd import sim as S
    from uhc_amd.agents import agent_dict
    from uhc_amd.data_loaders.dataset_amass_single import DatasetAMASSSingle
    from uhc_amd.data_loaders.synthetic import make_synthetic_amass
    from uhc_amd.smpllib import smpl_eval as E
    from uhc_amd.utils.config_utils.copycat_config import Config

    torch.set_default_dtype(torch.float64)
    cfg = Config(cfg_id="copycat_mi355x", base_dir=tempfile.mkdtemp(prefix="bench_surface_"))
    cfg.n_env, cfg.min_batch_size, cfg.num_optim_epoch, cfg.no_log, cfg.save_n_epochs = args.n_env, args.n_env * 4, 1, True, 10 ** 6
    cfg.bank_build, cfg.eval_build, cfg.fail_safe = "device", "device", False
    specs = dict(cfg.data_specs)
    specs["file_path"] = "synthetic"
    loader = DatasetAMASSSingle(specs, "train", pickle_data=make_synthetic_amass(args.clips, seed=4, t_range=(max(args.frames - 20, 3), args.frames + 20)))
    agent = agent_dict[cfg.agent_name](cfg, torch.float64, torch.device("cuda", 0), data_loader=loader)
    agent.optimize_policy(0, save_model=False)  # (fills the running filter)
    keys = list(loader.data_keys)
    rs = agent.running_state.rs
    st = copy.deepcopy(rs.__getstate__())
    sync = torch.cuda.synchronize

    def one_pass(surface):
        rs._n = st["_n"]
        rs._M[...], rs._S[...] = st["_M"], st["_S"]
        rs._host_changed()
        cfg.eval_surface = surface
        sync()
        t0 = time.perf_counter()
        out = agent.eval_seqs(keys, loader)
        sync()
        return time.perf_counter() - t0, out

    dev_name = torch.cuda.get_device_name(0)
    res = dict(clips=args.clips, n_env=args.n_env, frames=int(sum(loader.get_sample_len_from_key(k) for k in keys)), device=dev_name)
    lines = [f"surface metrics: {args.clips} synthetic clips, {res['frames']} frames, n_env {args.n_env}, fail_safe off  [{dev_name}]"]
    # ---- (a)
    times, outs = {}, {}
    for surface in (False, True):
        one_pass(surface)  # warm-up (the first pass also builds the evaluation env, its bank and the vertex tables)
    for surface in (False, True) * args.repeats:  # alternating: other work shares the machine
        t, outs[surface] = one_pass(surface)
        times.setdefault(surface, []).append(t)
    rows = int(sum(outs[True][k]["pred"].shape[0] for k in keys))
    same = all(np.array_equal(outs[True][k][n], outs[False][k][n]) for k in keys for n in outs[False][k])
    t_off, t_on = statistics.median(times[False]), statistics.median(times[True])
    chunks = -(-len(keys) // min(len(keys), args.n_env))
    steps = chunks * max(loader.get_sample_len_from_key(k) for k in keys)  # (a lower bound of the control steps of a pass: max(lens) per chunk, then blocks of 16)
    res["eval_seqs"] = dict(off_s=t_off, on_s=t_on, added_s=t_on - t_off, added_share=(t_on - t_off) / t_off, off_all_s=times[False], on_all_s=times[True], rows=rows,
                            other_results_equal=bool(same), mean_pentration_mm=float(np.mean([outs[True][k]["pentration"] for k in keys])),
                            mean_skate_mm=float(np.mean([outs[True][k]["skate"] for k in keys])))
    lines += [f"(a) eval_seqs, eval_build='device', {rows} recorded rows:",
              f"    eval_surface off {t_off:8.3f} s   ({', '.join('%.3f' % t for t in times[False])})",
              f"    eval_surface on  {t_on:8.3f} s   ({', '.join('%.3f' % t for t in times[True])})   on - off = {1e3 * (t_on - t_off):.1f} ms = {100 * (t_on - t_off) / t_off:.1f} % "
              f"of the pass;  every other result array equal: {same}"]

    # ---- (b) the launch alone: the clips' expert poses in a pose record of the pass's shape
    ev = next(iter(agent._eval_envs.values()))
    frames, starts = ev.env._bank[0], ev.env._bank[1].cpu().numpy()
    dev = frames.device
    n = min(len(keys), args.n_env)
    lens = np.array([loader.get_sample_len_from_key(k) for k in keys[:n]])
    rec = EO.Record(n, 2 * int(lens.max()) + 2, ev.qpos_lim, dev, poses=True)
    for e, k in enumerate(keys[:n]):
        f = frames[int(starts[ev._clip_index[k]]):int(starts[ev._clip_index[k]]) + int(lens[e])]
        rec.rows[e] = int(lens[e])
        rec.pred_pose[e, :lens[e], :72], rec.pred_pose[e, :lens[e], 72:] = f[:, EO.FR_WBPOS:EO.FR_WBPOS + 72], f[:, EO.FR_WBQUAT:EO.FR_WBQUAT + 96]
    surface = EO.Surface(list(ev.body_models), body_lim=ev.body_lim)
    n_rows, V = int(lens.sum()), surface.n_vert

    def events(fn, reps=20, inner=1):
        for _ in range(3):
            fn()
        sync()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / inner)
        return statistics.median(ms), min(ms), max(ms)

    row_out = torch.empty(n * rec.row_cap, 4, dtype=torch.float64, device=dev)
    means = torch.empty(n, 4, dtype=torch.float64, device=dev)
    k_ms = events(lambda: EO.surface_metrics_of_record(surface, rec, row_out=row_out, seq_means=means))
    # the bytes one launch reads: every row's pose twice (as its own and as the row before's next), the vertex tables once per row (from cache)
    read_rows = rec.pred_pose.view(-1, EO.POSE_ROW)[:n_rows].contiguous()
    dst = torch.empty_like(read_rows)
    c_ms = events(lambda: dst.copy_(read_rows))

    def host():
        t0 = time.perf_counter()
        pose = rec.pred_pose.cpu().numpy()  # (the copy the host path would have to make)
        info = {"floor_z": 0}
        tab = surface.tables[0]
        for e in range(n):
            vert = E.hull_vertices(tab, pose[e, :lens[e], :72], pose[e, :lens[e], 72:])
            E.compute_penetration(vert, info), E.compute_skate(vert, info), E.compute_float(vert, info), E.compute_contact(vert, info)
        return time.perf_counter() - t0

    host()
    h_s = [host() for _ in range(args.repeats)]
    flop_row = V * 2 * 20 + 24 * 2 * 45  # two transforms of 18 flops and the height / slide terms per vertex; two quaternion -> matrix conversions per body
    res["launch"] = dict(envs=n, rows=n_rows, n_vert=V, kernel_ms=k_ms[0], kernel_min_ms=k_ms[1], kernel_max_ms=k_ms[2], host_s=statistics.median(h_s), host_all_s=h_s,
                         host_over_kernel=statistics.median(h_s) * 1e3 / k_ms[0], copy_ms=c_ms[0], pose_bytes=int(read_rows.numel() * 8),
                         gflops=n_rows * flop_row / (k_ms[0] * 1e-3) / 1e9)
    lines += [f"(b) uhc_surface_metrics alone, {n} sequences, {n_rows} rows x {V} vertices (row cap {rec.row_cap}):",
              f"    device  {k_ms[0]:8.3f} ms (min {k_ms[1]:.3f}, max {k_ms[2]:.3f}; median of 20, HIP events; {res['launch']['gflops']:.0f} GFLOP/s float64 at {flop_row} flop a row)",
              f"    host    {statistics.median(h_s) * 1e3:8.1f} ms ({', '.join('%.1f' % (t * 1e3) for t in h_s)}; numpy, the device -> host copy of the poses included)   "
              f"host / device = {res['launch']['host_over_kernel']:.0f}",
              f"    a plain device copy of the {res['launch']['pose_bytes'] / 1e6:.1f} MB of poses it reads: {c_ms[0]:.3f} ms"]

    # ---- (c) record_pose beside a control step
    active = torch.ones(n, dtype=torch.int32, device=dev)
    rec.rows.zero_()
    xpos_f, xquat_f = ev.sim.field(S.F_XPOS), ev.sim.field(S.F_XQUAT)
    if xpos_f.shape[0] == n:
        p_ms = events(lambda: EO.record_pose(rec, 0, xpos_f, xquat_f, active), inner=50)
        step_ms = t_off * 1e3 / steps
        res["record_pose"] = dict(us=p_ms[0] * 1e3, step_ms_upper=step_ms, share_of_step_lower=p_ms[0] / step_ms)
        lines.append(f"(c) uhc_eval_record_pose alone, {n} envs: {p_ms[0] * 1e3:.1f} us a launch (median of 20 runs of 50; a pass makes two a step);  a control step of pass (a) "
                     f"takes at most {step_ms:.2f} ms (pass time / {steps} steps): two launches are at least {100 * 2 * p_ms[0] / step_ms:.2f} % of it")
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    surface.close()
    agent.env.close()


if __name__ == "__main__":
    main()
