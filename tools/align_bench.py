#!/usr/bin/env python
"""TSDF alignment throughput (include/rgbid_tsdf_align.h) on the volumes of tools/tsdf_bench.py and tools/raycast_bench.py: the batch's
keyframes (n synthesised 640 x 480 export blocks with random poses near the origin, one room) are integrated into a cube of `side`^3 voxels
over the box of the batch's cloud, and all n views are aligned to the volume from their own poses in one call of `iterations` Gauss-Newton
iterations at stride 1.  The call is timed with the library's HIP events (rgbid_tsdf_align_timing: one event after every launch): the
median of `reps` calls after `warmup`; one JSON line per (batch, side), printed and written to --out, with

    system_us           one k_tsdf_align_system launch over all views (the call's system time / iterations)
    solve_us            one k_tsdf_align_solve launch over all views (the call's solve time / iterations)
    pixels_per_s        views x rows x cols over system_us
    used                used pixels of the first system, over all views; running: the views that took every iteration
    raycast_us          one ray cast of the same views from the same volume with step = voxel, in the same process, its own HIP events: the
                        only existing pass that samples the volume per pixel.  Nothing about a time or a ratio is asserted: the kernels have
                        no parent to compare with, and the synthetic batches' surface is noise

    python tools/align_bench.py [--sizes 16] [--sides 256 512] [--iterations 10] [--reps 10] [--out profiles/align_bench.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16])
    ap.add_argument("--sides", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--mode", choices=["novel", "all"], default="novel")
    ap.add_argument("--trunc-voxels", type=float, default=4.0)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from cloud_bench import synth_blocks
    from voxel_bench import random_rotation
    from rgbid import cloud as CL
    from rgbid import device
    from rgbid import tsdf as TS
    rows, cols = args.rows, args.cols
    K = (525.0 * cols / 640, 525.0 * rows / 480, cols / 2 - 0.5, rows / 2 - 0.5)
    N = rows * cols
    levels = TS.align_levels_arg(((1, args.iterations),))
    lines = []
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = device.Context(0)
        for n in args.sizes:
            buf = synth_blocks(n, rows, cols, 1000 + n)
            rng = np.random.default_rng(n)
            R = np.stack([random_rotation(rng, 0.3) for _ in range(n)])       # one room: the batch of tools/tsdf_bench.py
            t = rng.uniform(-0.2, 0.2, (n, 3))
            cl = CL.Cloud(ctx, rows, cols, n)
            pts, offsets = cl.build([CL.source(buf[k].data_ptr(), R[k], t[k]) for k in range(n)], K, args.mode)
            cl.close()
            planes = [buf[k, 4 * N:8 * N].view(torch.float32).view(rows, cols) for k in range(n)]
            colours = [buf[k, N:4 * N].view(rows, cols, 3) for k in range(n)]
            box = np.array(TS.cloud_bounds(pts))
            for side in args.sides:
                voxel = float((box[3:] - box[:3]).max() / (side - 1))
                vol = TS.Volume(ctx, side ** 3, n)
                vol.configure(side, side, side, [float(v) for v in box[:3]], voxel, args.trunc_voxels * voxel)
                vol.integrate(planes, colours, R, t, K, rows, cols)
                vol.timing(True)
                sys_t, sol_t, cast_t, res = [], [], [], None
                for k in range(args.warmup + args.reps):
                    res = vol.align(planes, R, t, K, rows, cols, levels, eps=1e-300)       # no view meets eps: every launch has all its views
                    ms = vol.align_timing(True)
                    vol.raycast(R, t, K, rows, cols, outputs=("depth",))                   # step = voxel
                    cast = vol.raycast_timing(True)
                    if k >= args.warmup:
                        sys_t.append(ms["system"] * 1e-3); sol_t.append(ms["solve"] * 1e-3); cast_t.append(cast * 1e-3)
                vol.timing(False)
                vol.close()
                system, solve = float(np.median(sys_t)) / args.iterations, float(np.median(sol_t)) / args.iterations
                line = {"keyframes": n, "mode": args.mode, "views": n, "rows": rows, "cols": cols, "side": side, "voxels": side ** 3, "voxel_m": voxel,
                        "stride": 1, "iterations": args.iterations, "system_us": system * 1e6, "solve_us": solve * 1e6, "pixels_per_s": n * N / system,
                        "used": int(res["used"][:, 0].sum()), "running": int((res["iterations"] == args.iterations).sum()),
                        "raycast_us": float(np.median(cast_t)) * 1e6, "reps": args.reps, "library": os.path.relpath(TS._lib.LIB_PATH, ROOT),
                        "device": torch.cuda.get_device_name(0)}
                print(json.dumps(line), flush=True)
                lines.append(line)
                torch.cuda.empty_cache()
            del pts, buf, planes, colours
            torch.cuda.empty_cache()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
