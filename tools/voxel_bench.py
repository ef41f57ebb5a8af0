#!/usr/bin/env python
"""Voxel-grid filter throughput (include/rgbid_voxel.h) on real Cloud.build outputs: batches of n synthesised 640 x 480 export blocks
(tools/cloud_bench.py synth_blocks: ~70 % valid pixels, overlap mask 0 on half of them) placed with random poses near the origin, in
the novel and the all mode, filtered at a 1 cm leaf.  Each stage is timed with the library's HIP events (rgbid_voxel_timing) after
warm-up; one JSON line per (batch, mode) with the median microseconds per stage, points/s, the largest voxel's member count (the emit
runs one thread per voxel) and the fraction of 8 TB/s each stage reaches on its algorithmic bytes:

    n records in, F finite, R voxels (runs), V voxels out, k = key bytes (4 or 8), P = radix passes (8 key bits each)
    box   32 n          every 32-byte record is needed (x y z lie in each; 4 records share a 128-byte line)
    keys  32 n + (k + 4) n                   read the records, write (key, index)
    sort  P (k n + 2 (k + 4) n)              per pass: the histogram reads the keys, the scatter reads and writes (key, index)
    runs  2 k F + 4 R (+ 8 R + 8 V with min_points > 1)   the head test reads each key twice (its own and the previous), starts written
    emit  8 V + 36 F + 32 V                  voxel bounds, the sorted index and the 32-byte record of every member, one record out

    python tools/voxel_bench.py [--sizes 16 256] [--modes novel all] [--leaf 0.01] [--reps 10]
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

PEAK_BPS = 8.0e12


def random_rotation(rng, max_angle):
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    a = rng.uniform(0, max_angle)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--modes", nargs="+", choices=["novel", "all"], default=["novel", "all"])
    ap.add_argument("--leaf", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--cols", type=int, default=640)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from cloud_bench import synth_blocks
    from rgbid import cloud as CL
    from rgbid import device
    from rgbid import voxel as VX
    rows, cols = args.rows, args.cols
    K = (525.0 * cols / 640, 525.0 * rows / 480, cols / 2 - 0.5, rows / 2 - 0.5)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = device.Context(0)
        for n in args.sizes:
            buf = synth_blocks(n, rows, cols, 1000 + n)
            rng = np.random.default_rng(n)
            srcs = [CL.source(buf[k].data_ptr(), random_rotation(rng, 0.3), rng.uniform(-0.2, 0.2, 3)) for k in range(n)]   # one room
            cl = CL.Cloud(ctx, rows, cols, n)
            for mode in args.modes:
                pts, _ = cl.build(srcs, K, mode)
                M = pts.shape[0]
                vg = VX.VoxelGrid(ctx, M)
                vg.timing(True)
                plan = vg.plan(pts, args.leaf)
                out = torch.empty((plan.voxels, 32), dtype=torch.uint8, device="cuda")
                for _ in range(args.warmup):
                    vg.plan(pts, args.leaf); vg.emit(out); ctx.sync()
                t = {s: [] for s in VX.STAGES}
                for _ in range(args.reps):
                    vg.plan(pts, args.leaf); vg.emit(out); ctx.sync()
                    for s, ms in vg.timing(True).items():
                        t[s].append(ms * 1e-3)
                vg.close()
                med = {s: float(np.median(v)) for s, v in t.items()}
                counts = VX.as_numpy(out)["count"]
                F, R, V = plan.finite, plan.runs, plan.voxels
                kb = 4 if plan.div_b[0] * plan.div_b[1] * plan.div_b[2] < (1 << 32) else 8
                passes = (int(np.prod(plan.div_b, dtype=np.float64)).bit_length() + 7) // 8
                model = {"box": 32 * M, "keys": 32 * M + (kb + 4) * M, "sort": passes * (kb * M + 2 * (kb + 4) * M),
                         "runs": 2 * kb * F + 4 * R, "emit": 8 * V + 36 * F + 32 * V}
                total = sum(med.values())
                print(json.dumps({
                    "keyframes": n, "mode": mode, "leaf": args.leaf, "points": M, "finite": F, "voxels": V, "key_bytes": kb, "passes": passes,
                    "stage_us": {s: med[s] * 1e6 for s in VX.STAGES}, "total_us": total * 1e6, "points_per_s": M / total,
                    "frac_8TBps": {s: model[s] / med[s] / PEAK_BPS for s in VX.STAGES}, "bytes_per_point": sum(model.values()) / M,
                    "largest_voxel": int(counts.max()), "mean_members": F / max(V, 1), "reps": args.reps,
                }), flush=True)
                del pts, out
                torch.cuda.empty_cache()
            cl.close()
            del buf
            torch.cuda.empty_cache()
        ctx.close()


if __name__ == "__main__":
    main()
