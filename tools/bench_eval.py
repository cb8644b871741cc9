#!/usr/bin/env python3
"""AgentCopycat.eval_seqs with cfg.eval_build = "host" against "device" on the same agent and the same clips (synthetic, one env per clip):

  (a) wall time of eval_seqs, host path: per control step copies of qpos / xpos / the expert frame / done / reward / percent to the host and Python
      lists per clip, compute_metrics in numpy at the end;
  (b) wall time of eval_seqs, device path: uhc_eval_record appends on the device, uhc_eval_metrics scores, one copy per chunk;
      both with cfg.fail_safe off (no device -> host read in the device path's step loop) and on (one read per step: the envs to teleport);
  (c) uhc_eval_metrics alone (HIP events) on a record of the shape (b) produced.

Every figure: one warm-up pass first, a device synchronise inside the timed window, the median of the repeats; the running filter's state is put back
before every pass, so that all passes run the same episodes.  The largest difference between the two paths' result arrays is printed beside the times.

  python tools/bench_eval.py [--clips 256] [--frames 300] [--n-env 256] [--repeats 3] [--out profiles/...txt]
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
        raise SystemExit("bench_eval: needs the GPU (a time taken elsewhere says nothing about it)")
    from uhc_amd import eval_ops as EO
    from uhc_amd.agents import agent_dict
    from uhc_amd.data_loaders.dataset_amass_single import DatasetAMASSSingle
    from uhc_amd.data_loaders.synthetic import make_synthetic_amass
    from uhc_amd.utils.config_utils.copycat_config import Config

    torch.set_default_dtype(torch.float64)
    cfg = Config(cfg_id="copycat_mi355x", base_dir=tempfile.mkdtemp(prefix="bench_eval_"))
    cfg.n_env, cfg.min_batch_size, cfg.num_optim_epoch, cfg.no_log, cfg.save_n_epochs = args.n_env, args.n_env * 4, 1, True, 10 ** 6
    cfg.bank_build = "device"
    specs = dict(cfg.data_specs)
    specs["file_path"] = "synthetic"
    loader = DatasetAMASSSingle(specs, "train", pickle_data=make_synthetic_amass(args.clips, seed=4, t_range=(max(args.frames - 20, 3), args.frames + 20)))
    agent = agent_dict[cfg.agent_name](cfg, torch.float64, torch.device("cuda", 0), data_loader=loader)
    agent.optimize_policy(0, save_model=False)  # (fills the running filter)
    keys = list(loader.data_keys)
    rs = agent.running_state.rs
    st = copy.deepcopy(rs.__getstate__())
    sync = torch.cuda.synchronize

    def one_pass(build):
        rs._n = st["_n"]
        rs._M[...], rs._S[...] = st["_M"], st["_S"]
        rs._host_changed()
        cfg.eval_build = build
        sync()
        t0 = time.perf_counter()
        out = agent.eval_seqs(keys, loader)
        sync()
        return time.perf_counter() - t0, out

    res = dict(clips=args.clips, n_env=args.n_env, frames=int(sum(loader.get_sample_len_from_key(k) for k in keys)), device=torch.cuda.get_device_name(0))
    lines = [f"eval_seqs: {args.clips} synthetic clips, {res['frames']} frames, n_env {args.n_env}  [{res['device']}]"]
    last = None
    for fs in (False, True):
        cfg.fail_safe = fs
        times, outs = {}, {}
        for build in ("host", "device"):
            one_pass(build)  # warm-up (the first pass also builds the evaluation env and its bank)
        for build in ("host", "device") * args.repeats:  # alternating: other work shares the machine
            t, outs[build] = one_pass(build)
            times.setdefault(build, []).append(t)
        diff = max((float(np.abs(np.asarray(outs["host"][k][n], dtype=float) - np.asarray(outs["device"][k][n], dtype=float)).max())
                    for k in keys for n in outs["host"][k] if np.size(outs["host"][k][n])), default=0.0)
        rows = int(sum(outs["device"][k]["pred"].shape[0] for k in keys))
        th, td = statistics.median(times["host"]), statistics.median(times["device"])
        tag = "on" if fs else "off"
        res[f"fail_safe_{tag}"] = dict(host_s=th, device_s=td, host_over_device=th / td, host_all_s=times["host"], device_all_s=times["device"], rows=rows,
                                       max_abs_diff_host_device=diff, clips_with_fail_safe=int(sum(outs["device"][k]["fail_safe"] for k in keys)))
        lines += [f"fail_safe {tag}: {rows} recorded rows, {res[f'fail_safe_{tag}']['clips_with_fail_safe']} clips teleported",
                  f"  (a) eval_build='host'   {th:8.3f} s   ({', '.join('%.3f' % t for t in times['host'])})",
                  f"  (b) eval_build='device' {td:8.3f} s   ({', '.join('%.3f' % t for t in times['device'])})   host / device = {th / td:.2f};  "
                  f"max |host - device| over every result array = {diff:.3e}"]
        last = outs["device"]

    # ---- (c) the metrics call alone, on a record shaped like the last pass's
    ev = next(iter(agent._eval_envs.values()))
    frames, starts = ev.env._bank[0], ev.env._bank[1].cpu().numpy()
    n = min(len(keys), args.n_env)
    lens = np.array([loader.get_sample_len_from_key(k) for k in keys[:n]])
    rec = EO.Record(n, 2 * int(lens.max()) + 2, ev.qpos_lim, frames.device)
    for e, k in enumerate(keys[:n]):
        T = last[k]["pred"].shape[0]
        rec.rows[e] = T
        rec.pred_qpos[e, :T] = torch.from_numpy(last[k]["pred"]).to(frames.device)
        rec.pred_jpos[e, :T] = torch.from_numpy(last[k]["pred_jpos"]).to(frames.device)
        rec.gt_frame[e, :T] = torch.from_numpy(starts[ev._clip_index[k]] + np.minimum(np.arange(T), lens[e] - 1)).to(frames.device)
    rm = torch.empty(n, rec.row_cap, 6, dtype=torch.float64, device=frames.device)
    cm = torch.empty(n, 6, dtype=torch.float64, device=frames.device)
    for _ in range(3):
        EO.metrics(rec, frames, rm, cm)
    sync()
    ms = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        EO.metrics(rec, frames, rm, cm)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    n_rows = int(rec.rows.sum().item())
    res["metrics_call"] = dict(envs=n, rows=n_rows, ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))
    lines.append(f"(c) uhc_eval_metrics alone, {n} envs, {n_rows} rows: {statistics.median(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}; median of 20, HIP events)")
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    agent.env.close()


if __name__ == "__main__":
    main()
