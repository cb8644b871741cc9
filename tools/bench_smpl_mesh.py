#!/usr/bin/env python3
"""What the SMPL mesh kernel (uhc_smpl_mesh: vertices, joints and contact quality of posed SMPL bodies) costs on one MI355X, on a synthetic model of the real
size (6 890 vertices, 24 joints, at most 4 skin weights a vertex), float64:

  (a) metrics only, a record of --seqs sequences x ~--frames rows (pen / skate / float / contact per row, means per sequence; no vertex leaves the kernel);
  (b) vertices out for --live rows, one row per sequence: a live batch, one frame per env;
  (c) one row.

Each against three baselines on the same inputs:
  torch   a chunked library route on the device: Rodrigues, torch.matmul for the pose blend shapes, the chain, an einsum for the skinning, masked reductions
          for the metrics chunk by chunk (one row carried over for the skate) -- the largest chunk of rows whose [rows x 6890 x 12] blend of transforms
          fits --chunk-mb;
  host    smpl_mesh.lbs_numpy + smpl_eval.compute_* with the copy of poses and translations to the host; for (a) on --host-seqs sequences, scaled to all;
  copy    a plain device copy of the inputs the kernel reads.

One process, a warm-up first, kernel and torch route alternate, a device synchronise inside every timed window (HIP events), medians with their ranges.

  python tools/bench_smpl_mesh.py [--seqs 256] [--frames 300] [--live 1024] [--repeats 7] [--out profiles/...txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
V = 6890


def synthetic_model(rng):
    from uhc_amd.smpllib.smpl_mesh import model_from_tables
    from uhc_amd.smpllib.smpl_robot import SMPL_PARENTS
    skel = np.cumsum(rng.normal(scale=0.15, size=(24, 3)), axis=0) + [0, 0, 1.0]
    owner = rng.integers(0, 24, size=V)
    weights = np.zeros((V, 24))
    for k in range(4):
        weights[np.arange(V), (owner + 5 * k) % 24] += rng.uniform(0.1, 1.0, size=V)
    weights /= weights.sum(axis=1, keepdims=True)
    jr = np.zeros((24, V))
    for j in range(24):
        idx = rng.choice(V, size=32, replace=False)
        jr[j, idx] = rng.dirichlet(np.ones(32))
    return model_from_tables(dict(v_template=skel[owner] + rng.normal(scale=0.05, size=(V, 3)), shapedirs=rng.normal(scale=1e-2, size=(V, 3, 10)),
                                  posedirs=rng.normal(scale=1e-2, size=(V, 3, 207)), J_regressor=jr, weights=weights,
                                  kintree_table=np.stack([np.array(SMPL_PARENTS) % 2 ** 32, np.arange(24)]).astype(np.uint32)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--frames", type=int, default=300, help="sequence lengths are drawn from [frames - 20, frames + 20]")
    ap.add_argument("--live", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-seqs", type=int, default=2)
    ap.add_argument("--chunk-mb", type=int, default=4096)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_smpl_mesh: needs the GPU (a time taken elsewhere says nothing about it)")
    from uhc_amd import eval_ops as EO
    from uhc_amd.smpllib import smpl_mesh as SM
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(15)
    model = synthetic_model(rng)
    mesh = EO.SmplMesh([model])
    up = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(dev, dt)
    tm = {k: up(model[k]) for k in ("v_template", "shapedirs", "J_regressor", "weights")}
    tm["posedirs_t"] = up(model["posedirs"].reshape(V * 3, 207).T)  # [207][3 V]
    parents = [int(p) for p in model["parents"]]

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def torch_route(pose, trans, seq_of, row_of, betas, want_vert, metrics, chunk):
        """the library route: per sequence shapes, then chunks of rows (seq_of / row_of: the sequence and the global row of every row, made once outside)"""
        v_shaped = tm["v_template"][None] + torch.einsum("vcb,sb->svc", tm["shapedirs"], betas)
        J = torch.einsum("jv,svc->sjc", tm["J_regressor"], v_shaped)
        n = row_of.numel()
        outs, red, carry = [], [], None
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        for c0 in range(0, n, chunk):
            ri, si = row_of[c0:c0 + chunk], seq_of[c0:c0 + chunk]
            r = pose[ri].view(-1, 24, 3)
            a = (r + 1e-8).norm(dim=-1, keepdim=True)
            d = r / a
            K = torch.zeros(r.shape[0], 24, 3, 3, dtype=torch.float64, device=dev)
            K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -d[..., 2], d[..., 1], d[..., 2], -d[..., 0], -d[..., 1], d[..., 0]
            R = torch.eye(3, dtype=torch.float64, device=dev) + torch.sin(a)[..., None] * K + (1 - torch.cos(a))[..., None] * (K @ K)
            feat = (R[:, 1:] - torch.eye(3, dtype=torch.float64, device=dev)).reshape(-1, 207)
            v_posed = v_shaped[si] + torch.matmul(feat, tm["posedirs_t"]).view(-1, V, 3)
            Js = J[si]
            GR, Gt = [None] * 24, [None] * 24
            for j in range(24):
                p = parents[j]
                if p < 0:
                    GR[j], Gt[j] = R[:, j], Js[:, j]
                else:
                    GR[j] = GR[p] @ R[:, j]
                    Gt[j] = torch.einsum("tab,tb->ta", GR[p], Js[:, j] - Js[:, p]) + Gt[p]
            GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)
            A = torch.cat([GR, (Gt - torch.einsum("tjab,tjb->tja", GR, Js))[..., None]], -1).reshape(-1, 24, 12)
            T = torch.einsum("vj,tjk->tvk", tm["weights"], A).view(-1, V, 3, 4)
            vert = torch.einsum("tvab,tvb->tva", T[..., :3], v_posed) + T[..., 3] + trans[ri][:, None]
            if want_vert:
                outs.append(vert)
            if metrics:  # reduced chunk by chunk: four numbers a row stay, and the chunk's last row for the skate of the next chunk's first pair
                h, xy = vert[..., 2], vert[..., :2]
                under, touch = h < 0, h <= 0
                pen = torch.where(under.any(1), -(h * under).sum(1) / under.sum(1).clamp(min=1) * 1000, zero)
                flt = torch.where((h > 0).all(1), h.min(1).values * 1000, zero)
                if carry is not None:
                    touch2, xy2 = torch.cat([carry[0], touch]), torch.cat([carry[1], xy])
                else:
                    touch2, xy2 = touch, xy
                both = touch2[:-1] & touch2[1:]
                sl = ((xy2[1:] - xy2[:-1]) ** 2).sum(-1).sqrt()
                skate = torch.where(both.any(1), (sl * both).sum(1) / both.sum(1).clamp(min=1) * 1000, zero)  # (pairs across sequence ends are not cut out: a little less work than the kernel's)
                red.append((pen, skate, flt, touch.sum(1)))
                carry = (touch[-1:], xy[-1:])
        if not metrics:
            return torch.cat(outs)
        return tuple(torch.cat([r[k] for r in red]) for k in range(4))

    def measure(name, pose, trans, start, rows, betas, want, chunk, host_seqs):
        n_rows, n_seq = int(rows.sum().item()), rows.numel()
        metrics, want_vert = "metrics" in want, "vertices" in want
        out = {}
        if want_vert:
            out["vertices"] = torch.empty(pose.shape[0], V, 3, dtype=torch.float64, device=dev)
        cap = int(rows.max().item())
        kern = lambda: EO.smpl_mesh(mesh, pose, trans, start, rows, betas, want=want, row_cap=cap, out=out)
        seq_of = torch.repeat_interleave(torch.arange(n_seq, device=dev), rows.long())
        row_of = torch.cat([torch.arange(int(s), int(s) + int(r), device=dev) for s, r in zip(start.tolist(), rows.tolist())])
        lib = lambda: torch_route(pose, trans, seq_of, row_of, betas, want_vert, metrics, chunk)
        cp_src = [pose, trans, betas]
        cp_dst = [torch.empty_like(t) for t in cp_src]
        copy = lambda: [d.copy_(s) for d, s in zip(cp_dst, cp_src)]
        for fn in (kern, lib, copy):  # warm-up
            fn()
        sync()
        k_ms, l_ms, c_ms = [], [], []
        for _ in range(args.repeats):  # alternating: other work shares the machine
            k_ms.append(events(kern)), l_ms.append(events(lib)), c_ms.append(events(copy))

        def host():
            t0 = time.perf_counter()
            p, t = pose.cpu().numpy(), trans.cpu().numpy()
            for s in range(host_seqs):
                g0, T = int(start[s].item()), int(rows[s].item())
                vert, _ = SM.lbs_numpy(model, p[g0:g0 + T], betas[s].cpu().numpy(), t[g0:g0 + T])
                if metrics:
                    SM.mesh_metrics_numpy(vert, 0.0)
            return (time.perf_counter() - t0) * 1e3

        host()
        host_rows = int(rows[:host_seqs].sum().item())
        h_ms = [host() * n_rows / host_rows for _ in range(3)]
        med, rng_ = statistics.median, lambda x: f"{min(x):.3f} .. {max(x):.3f}"
        spread = max(l_ms) - min(l_ms)
        flop = n_rows * (2.0 * 207 * 3 * V + V * (24 * 4 + 18 + 10))  # the pose blend product; skinning at four weights a vertex, the point transform, the metric terms
        r = dict(workload=name, seqs=n_seq, rows=n_rows, want=list(want), kernel_ms=med(k_ms), kernel_all_ms=k_ms, torch_ms=med(l_ms), torch_all_ms=l_ms, torch_chunk_rows=chunk,
                 torch_spread_ms=spread, torch_minus_kernel_over_spread=(med(l_ms) - med(k_ms)) / spread if spread > 0 else float("inf"), host_ms=med(h_ms),
                 host_all_ms=h_ms, host_rows_measured=host_rows, copy_ms=med(c_ms), input_bytes=int(sum(t.numel() for t in cp_src) * 8),
                 kernel_tflops=flop / (med(k_ms) * 1e-3) / 1e12, rows_per_s=n_rows / (med(k_ms) * 1e-3))
        lines = [f"({name}) {n_seq} sequences, {n_rows} rows x {V} vertices, want = {', '.join(want)}:",
                 f"    uhc_smpl_mesh {med(k_ms):10.3f} ms ({rng_(k_ms)}; median of {args.repeats}, HIP events)   {r['kernel_tflops']:.2f} TFLOP/s float64, {r['rows_per_s']:.0f} rows/s",
                 f"    torch route   {med(l_ms):10.3f} ms ({rng_(l_ms)}; chunks of {chunk} rows)   torch / kernel = {med(l_ms) / med(k_ms):.2f};  torch - kernel = "
                 f"{med(l_ms) - med(k_ms):.3f} ms = {r['torch_minus_kernel_over_spread']:.1f} spreads of the torch route's repeats ({spread:.3f} ms)",
                 f"    host          {med(h_ms):10.1f} ms ({rng_(h_ms)}; lbs_numpy{' + compute_*' if metrics else ''}, copy included; measured on {host_rows} rows, scaled to {n_rows})"
                 f"   host / kernel = {med(h_ms) / med(k_ms):.0f}",
                 f"    a plain device copy of the {r['input_bytes'] / 1e6:.2f} MB of inputs: {med(c_ms):.3f} ms"]
        return r, lines

    chunk = max(1, int(args.chunk_mb * 1e6 / (V * 12 * 8 * 3)))  # the blend of transforms, the vertices and v_posed of a chunk live together
    name = torch.cuda.get_device_name(0)
    lines = [f"SMPL mesh: synthetic model of {V} vertices, 24 joints, four skin weights a vertex, float64  [{name}]"]
    res = dict(device=name, n_vert=V)

    def workload(n_seq, lens):
        start = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        n = int(lens.sum())
        d = rng.normal(size=(n, 24, 3))
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        pose = (d * rng.uniform(0, 0.6, size=(n, 24, 1))).reshape(n, 72)
        trans = np.concatenate([rng.normal(scale=0.3, size=(n, 2)), rng.uniform(-0.3, 0.1, size=(n, 1))], axis=1)
        return up(pose), up(trans), up(start, torch.int64), up(lens.astype(np.int32), torch.int32), up(rng.normal(size=(n_seq, 10)))

    for tag, n_seq, lens, want, hs in (("a", args.seqs, rng.integers(args.frames - 20, args.frames + 21, size=args.seqs), ("metrics",), args.host_seqs),
                                       ("b", args.live, np.ones(args.live, dtype=np.int64), ("vertices",), 32),
                                       ("c", 1, np.ones(1, dtype=np.int64), ("vertices", "metrics"), 1)):
        r, ls = measure(tag, *workload(n_seq, lens), want, chunk, min(hs, n_seq))
        res[tag] = r
        lines += ls
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    mesh.close()


if __name__ == "__main__":
    main()
