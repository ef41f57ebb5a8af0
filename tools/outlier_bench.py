#!/usr/bin/env python
"""Radius outlier filter throughput (include/rgbid_outlier.h) on real Cloud.build outputs: the batches of tools/voxel_bench.py (n
synthesised 640 x 480 export blocks placed with random poses near the origin, novel mode).  Each stage is timed with the library's HIP
events (rgbid_outlier_timing) after warm-up; one JSON line per (batch, cap) with the median microseconds per stage and

    candidates      the records in the 27 cells around every finite point (itself included): the distance evaluations of a walk that
                    never leaves early, counted here with torch from the same float32 grid
    evals_per_s     candidates / the count stage's time, reported for the run with cap = 2^31 (no early exit), where it is exact
    left_early      the share of the finite points whose count reached cap: they stopped walking there

and, beside them, the same batch's rgbid_voxel plan + emit time at a 1 cm leaf: the existing yardstick for a pass over the same records.

    python tools/outlier_bench.py [--sizes 16 256] [--radius 0.02] [--min-neighbours 4] [--reps 10] [--out profiles/outlier_bench.jsonl]
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


def candidates(pts, cell):
    """sum over the finite points of the population of the 27 cells around them, on the library's grid (floor(p * inv) in float32)"""
    xyz = pts.view(torch.float32).reshape(-1, 8)[:, :3]
    xyz = xyz[torch.isfinite(xyz).all(1)]
    inv = torch.tensor(1.0, dtype=torch.float32, device=xyz.device) / torch.tensor(float(cell), dtype=torch.float32, device=xyz.device)
    ijk = torch.floor(xyz * inv).to(torch.int64)
    ijk -= ijk.min(0).values - 1
    d = ijk.max(0).values + 2
    key = (ijk[:, 2] * d[1] + ijk[:, 1]) * d[0] + ijk[:, 0]
    ukeys, num = torch.unique(key, return_counts=True)
    total = 0
    for dk in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                nk = ukeys + ((dk * d[1] + dj) * d[0] + di)
                c = torch.searchsorted(ukeys, nk).clamp(max=len(ukeys) - 1)
                total += int((num * torch.where(ukeys[c] == nk, num[c], torch.zeros_like(num))).sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--radius", type=float, default=0.02)
    ap.add_argument("--min-neighbours", type=int, default=4)
    ap.add_argument("--leaf", type=float, default=0.01, help="the voxel yardstick's leaf")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outlier_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from cloud_bench import synth_blocks
    from voxel_bench import random_rotation
    from rgbid import cloud as CL
    from rgbid import device
    from rgbid import outlier as OL
    from rgbid import voxel as VX
    rows, cols = args.rows, args.cols
    K = (525.0 * cols / 640, 525.0 * rows / 480, cols / 2 - 0.5, rows / 2 - 0.5)
    lines = []
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = device.Context(0)
        for n in args.sizes:
            buf = synth_blocks(n, rows, cols, 1000 + n)
            rng = np.random.default_rng(n)
            srcs = [CL.source(buf[k].data_ptr(), random_rotation(rng, 0.3), rng.uniform(-0.2, 0.2, 3)) for k in range(n)]   # one room
            cl = CL.Cloud(ctx, rows, cols, n)
            pts, _ = cl.build(srcs, K, "novel")
            cl.close()
            M = pts.shape[0]
            cand = candidates(pts, OL.cell_size(args.radius))
            # the yardstick: the voxel filter's plan + emit over the same records
            vg = VX.VoxelGrid(ctx, M)
            vg.timing(True)
            vp = vg.plan(pts, args.leaf)
            vout = torch.empty((vp.voxels, 32), dtype=torch.uint8, device="cuda")
            vt = []
            for k in range(args.warmup + args.reps):
                vg.plan(pts, args.leaf); vg.emit(vout); ctx.sync()
                if k >= args.warmup:
                    vt.append(sum(vg.timing(True).values()) * 1e-3)
            vg.close()
            del vout
            voxel_s = float(np.median(vt))
            rf = OL.RadiusFilter(ctx, M)
            rf.timing(True)
            for cap in (args.min_neighbours, 1 << 31):
                plan = rf.plan(pts, args.radius, args.min_neighbours, cap)
                out = torch.empty((plan.kept, 32), dtype=torch.uint8, device="cuda")
                cnt = torch.empty((M,), dtype=torch.int32, device="cuda")
                t = {s: [] for s in OL.STAGES}
                for k in range(args.warmup + args.reps):
                    rf.plan(pts, args.radius, args.min_neighbours, cap); rf.emit(out); ctx.sync()
                    if k >= args.warmup:
                        for s, ms in rf.timing(True).items():
                            t[s].append(ms * 1e-3)
                rf.counts(cnt); ctx.sync()
                med = {s: float(np.median(v)) for s, v in t.items()}
                total = sum(med.values())
                c64 = cnt.to(torch.int64) & 0xffffffff
                line = {"keyframes": n, "points": M, "finite": plan.finite, "cells": plan.cells, "kept": plan.kept, "radius": args.radius,
                        "min_neighbours": args.min_neighbours, "cap": cap, "stage_us": {s: med[s] * 1e6 for s in OL.STAGES},
                        "total_us": total * 1e6, "points_per_s": M / total, "candidates": cand, "candidates_per_point": cand / max(plan.finite, 1),
                        "evals_per_s": cand / med["count"] if cap == 1 << 31 else None,
                        "left_early": float((c64 >= cap).sum()) / max(plan.finite, 1), "mean_count": float(c64.sum()) / max(plan.finite, 1),
                        "voxel_total_us": voxel_s * 1e6, "voxel_leaf": args.leaf, "ratio_to_voxel": total / voxel_s, "reps": args.reps}
                print(json.dumps(line), flush=True)
                lines.append(line)
                del out, cnt
            rf.close()
            del pts, buf
            torch.cuda.empty_cache()
        ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
