#!/usr/bin/env python
"""Consistency filter throughput (include/rgbid_consist.h) on real Cloud.build outputs: the batches of tools/voxel_bench.py and
tools/render_bench.py (n synthesised 640 x 480 export blocks placed with random poses near the origin, one room); the views are the
batch's own keyframes, V = n, with their own inverse-depth planes and owner ranges, and window half-width w.  Each stage is timed with the
library's HIP events (rgbid_consist_timing): the median of `reps` plan + emit calls after `warmup`; one JSON line per (batch, w), printed
and written to --out, with

    stage_us            count (view table upload, count and mark pass), scan (count and scan of the keep flags), emit
    pairs_per_s         records x views per second of the whole call
    gated_share         (record, view) pairs that passed the depth gate and the image test, of all pairs
    bytes_min           the algorithmic minimum of the count stage: 16 B per record read, 5 B written, 4 B per gated pair and window pixel
    splat_us            rgbid_render's splat at s = 0 over the same records and the first 16 views, in the same process: the one existing
                        pass that projects these records; splat_pairs_per_s is its records x views per second.
                        Nothing about the ratio is asserted

    python tools/consist_bench.py [--sizes 16 256] [--windows 0 1] [--reps 10] [--out profiles/consist_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rgbid-slam_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

SPLAT_VIEWS = 16


def splat_time(ctx, pts, R, t, K, rows, cols, warmup, reps):
    """median seconds of the renderer's splat stage at s = 0 over pts and the given views"""
    from rgbid import render as RD
    rd = RD.Renderer(ctx, pts.shape[0], rows * cols * len(R))
    rd.timing(True)
    ts = []
    for k in range(warmup + reps):
        rd.render(pts, R, t, K, rows, cols, 0, outputs=("depth",))
        ms = rd.timing(True)
        if k >= warmup:
            ts.append(ms["splat"] * 1e-3)
    rd.close()
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--windows", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--mode", choices=["novel", "all"], default="novel")
    ap.add_argument("--tol-rel", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consist_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from cloud_bench import synth_blocks
    from voxel_bench import random_rotation
    from rgbid import cloud as CL
    from rgbid import consist as CF
    from rgbid import device
    rows, cols = args.rows, args.cols
    K = (525.0 * cols / 640, 525.0 * rows / 480, cols / 2 - 0.5, rows / 2 - 0.5)
    N = rows * cols
    lines = []
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = device.Context(0)
        for n in args.sizes:
            buf = synth_blocks(n, rows, cols, 1000 + n)
            rng = np.random.default_rng(n)
            R = np.stack([random_rotation(rng, 0.3) for _ in range(n)])       # one room
            t = rng.uniform(-0.2, 0.2, (n, 3))
            cl = CL.Cloud(ctx, rows, cols, n)
            pts, offsets = cl.build([CL.source(buf[k].data_ptr(), R[k], t[k]) for k in range(n)], K, args.mode)
            cl.close()
            planes = [buf[k, 4 * N:8 * N].view(torch.float32).view(rows, cols) for k in range(n)]     # the blocks' inverse depth, in place
            M = pts.shape[0]
            splat = splat_time(ctx, pts, R[:SPLAT_VIEWS], t[:SPLAT_VIEWS], K, rows, cols, args.warmup, args.reps)
            nv = min(n, SPLAT_VIEWS)
            cf = CF.ConsistencyFilter(ctx, M, n)
            out = torch.empty((M, 32), dtype=torch.uint8, device="cuda")
            for w in args.windows:
                cf.timing(True)
                ts = {st: [] for st in CF.STAGES}
                for k in range(args.warmup + args.reps):
                    plan = cf.plan(pts, offsets, planes, R, t, K, rows, cols, tol_rel=args.tol_rel, window=w)
                    cf.emit(out); ctx.sync()
                    ms = cf.timing(True)
                    if k >= args.warmup:
                        for st, v in ms.items():
                            ts[st].append(v * 1e-3)
                cf.timing(False)
                med = {k: float(np.median(v)) for k, v in ts.items()}
                total = sum(med.values())
                bytes_min = 21 * M + 4 * plan.pairs * (2 * w + 1) ** 2
                line = {"keyframes": n, "mode": args.mode, "points": M, "views": n, "rows": rows, "cols": cols, "window": w, "tol_rel": args.tol_rel,
                        "stage_us": {k: med[k] * 1e6 for k in CF.STAGES}, "total_us": total * 1e6, "pairs_per_s": M * n / total,
                        "gated_pairs": plan.pairs, "gated_share": plan.pairs / (M * n), "kept": plan.kept, "contradicted": plan.contradicted,
                        "plane_bytes": 4 * N * n, "bytes_min": bytes_min, "count_bytes_per_s": bytes_min / med["count"],
                        "splat_views": nv, "splat_us": splat * 1e6, "splat_pairs_per_s": M * nv / splat,
                        "pairs_rate_over_splat": (M * n / med["count"]) / (M * nv / splat), "reps": args.reps,
                        "library": os.path.relpath(CF._lib.LIB_PATH, ROOT), "device": torch.cuda.get_device_name(0)}
                print(json.dumps(line), flush=True)
                lines.append(line)
            cf.close()
            del pts, buf, planes, out
            torch.cuda.empty_cache()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
