#!/usr/bin/env python
"""TSDF fusion and mesh extraction throughput (include/rgbid_tsdf.h) on the batches of tools/consist_bench.py (n synthesised 640 x 480
export blocks placed with random poses near the origin, one room): the views are the batch's keyframes with their own inverse-depth planes
and colour areas, the volume is a cube of `side`^3 voxels over the box of the batch's cloud.  Each stage is timed with the library's HIP
events (rgbid_tsdf_timing): the median of `reps` reset + integrate + extract calls after `warmup`; one JSON line per (batch, side), printed
and written to --out, with

    stage_us            integrate (view table upload and the launches of all views), scan (flags, counts and their scans), emit
    pairs_per_s         voxels x views per second of the integrate stage
    state_bytes_min     the algorithmic minimum of the integrate stage: D and counts read once (8 B per voxel), written once per touched
                        voxel (8 B), the colour sums read and written once per coloured voxel (24 B)
    state_bytes_moved   what the launches move: the same per launch of RGBID_TSDF_VIEW_CHUNK views (an upper estimate: a launch writes
                        only the voxels its own views touched); share_of_8TBs is that over the stage's time over 8 TB/s
    count_us            rgbid_consist's count stage at w = 0 over the batch's cloud and the same views, in the same process: the one
                        existing pass that projects into these planes; count_pairs_per_s is its records x views per
                        second.  Nothing about the ratio is asserted

    python tools/tsdf_bench.py [--sizes 16 256] [--sides 256 512] [--reps 10] [--out profiles/tsdf_bench.jsonl]
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


def count_time(ctx, pts, offsets, planes, R, t, K, rows, cols, warmup, reps):
    """median seconds of the consistency filter's count stage at w = 0 over pts and the given views"""
    from rgbid import consist as CF
    cf = CF.ConsistencyFilter(ctx, pts.shape[0], len(R))
    cf.timing(True)
    ts = []
    for k in range(warmup + reps):
        cf.plan(pts, offsets, planes, R, t, K, rows, cols, window=0)
        ms = cf.timing(True)
        if k >= warmup:
            ts.append(ms["count"] * 1e-3)
    cf.close()
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--sides", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--mode", choices=["novel", "all"], default="novel")
    ap.add_argument("--trunc-voxels", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_bench.jsonl"))
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
            colours = [buf[k, N:4 * N].view(rows, cols, 3) for k in range(n)]                         # and their colour areas
            M = pts.shape[0]
            count = count_time(ctx, pts, offsets, planes, R, t, K, rows, cols, args.warmup, args.reps)
            box = np.array(TS.cloud_bounds(pts))
            for side in args.sides:
                voxel = float((box[3:] - box[:3]).max() / (side - 1))
                trunc = args.trunc_voxels * voxel
                vol = TS.Volume(ctx, side ** 3, n)
                vol.configure(side, side, side, [float(v) for v in box[:3]], voxel, trunc)
                vol.timing(True)
                ts = {st: [] for st in TS.STAGES}
                for k in range(args.warmup + args.reps):
                    vol.reset()
                    vol.integrate(planes, colours, R, t, K, rows, cols)
                    verts, vcols, tris = vol.extract(1)
                    ms = vol.timing(True)
                    if k >= args.warmup:
                        for st, v in ms.items():
                            ts[st].append(v * 1e-3)
                vol.timing(False)
                _, counts, _ = vol.state()
                touched = int(((counts & 0xFFFF) != 0).sum().item()); coloured = int(((counts >> 16) != 0).sum().item())
                vol.close()
                med = {k: float(np.median(v)) for k, v in ts.items()}
                nvox = side ** 3
                launches = (n + TS.VIEW_CHUNK - 1) // TS.VIEW_CHUNK
                bytes_min = 8 * nvox + 8 * touched + 24 * coloured
                moved = launches * bytes_min
                line = {"keyframes": n, "mode": args.mode, "views": n, "rows": rows, "cols": cols, "side": side, "voxels": nvox, "voxel_m": voxel,
                        "trunc_m": trunc, "stage_us": {k: med[k] * 1e6 for k in TS.STAGES}, "pairs_per_s": nvox * n / med["integrate"],
                        "touched": touched, "coloured": coloured, "vertices": int(verts.shape[0]), "triangles": int(tris.shape[0]),
                        "launches": launches, "state_bytes_min": bytes_min, "state_bytes_moved": moved,
                        "share_of_8TBs": moved / med["integrate"] / 8e12, "extract_us": (med["scan"] + med["emit"]) * 1e6,
                        "points": M, "count_us": count * 1e6, "count_pairs_per_s": M * n / count,
                        "pairs_rate_over_count": (nvox * n / med["integrate"]) / (M * n / count), "reps": args.reps,
                        "library": os.path.relpath(TS._lib.LIB_PATH, ROOT), "device": torch.cuda.get_device_name(0)}
                print(json.dumps(line), flush=True)
                lines.append(line)
                del verts, vcols, tris, counts
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
