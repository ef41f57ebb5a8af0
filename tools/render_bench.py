#!/usr/bin/env python
"""Map renderer throughput (include/rgbid_render.h) on real Cloud.build outputs: the batches of tools/voxel_bench.py (n synthesised
640 x 480 export blocks placed with random poses near the origin, one room) seen from V cameras of 640 x 480 drawn from the same pose
distribution, with splat half-width s.  Each stage is timed with the library's HIP events (rgbid_render_timing): the median of `reps`
calls after `warmup`; one JSON line per (batch, V, s), printed and written to --out, with

    stage_us            clear, splat, resolve
    pairs_per_s         records x views per second of the whole call
    visible_share       (record, view) pairs that passed the depth gate and the image test, of all pairs
    atomic_share        attempted pixel writes that reached the 64-bit atomic (the others left at the plain load), from a counting call
    bytes_min           the algorithmic minimum per stage: clear 8 B per pixel and view; splat 32 B per record and launch (one launch per
                        16 views); resolve 8 B per pixel and view read, the requested planes written (depth 4 + colour 3 B), 32 B per
                        drawn pixel for its winner's record
    frac_8TBps          bytes_min / time / 8 TB/s per stage
    voxel_total_us      rgbid_voxel plan + emit (1 cm leaf) over the same records in the same process: the one existing pass over these
                        records to hold a time against (DESIGN.md sections 12, 15, 17); nothing about the ratio is asserted

    python tools/render_bench.py [--sizes 16 256] [--views 1 16] [--splats 0 1] [--reps 10] [--out profiles/render_bench.jsonl]
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
OUTPUTS = ("depth", "colour")
PLANE_BYTES = {"index": 4, "depth": 4, "colour": 3, "normal": 12}


def voxel_total(ctx, pts, leaf, warmup, reps):
    """median seconds of rgbid_voxel plan + emit over pts, the sum of its stages' medians as tools/voxel_bench.py forms it"""
    from rgbid import voxel as VX
    vg = VX.VoxelGrid(ctx, pts.shape[0])
    vg.timing(True)
    plan = vg.plan(pts, leaf)
    out = torch.empty((plan.voxels, 32), dtype=torch.uint8, device="cuda")
    t = {s: [] for s in VX.STAGES}
    for k in range(warmup + reps):
        vg.plan(pts, leaf); vg.emit(out); ctx.sync()
        ms = vg.timing(True)
        if k >= warmup:
            for s, v in ms.items():
                t[s].append(v * 1e-3)
    vg.close()
    return sum(float(np.median(v)) for v in t.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--views", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--splats", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--mode", choices=["novel", "all"], default="novel")
    ap.add_argument("--leaf", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from cloud_bench import synth_blocks
    from voxel_bench import random_rotation
    from rgbid import cloud as CL
    from rgbid import device
    from rgbid import render as RD
    rows, cols = args.rows, args.cols
    K = (525.0 * cols / 640, 525.0 * rows / 480, cols / 2 - 0.5, rows / 2 - 0.5)
    npix = rows * cols
    lines = []
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = device.Context(0)
        for n in args.sizes:
            buf = synth_blocks(n, rows, cols, 1000 + n)
            rng = np.random.default_rng(n)
            srcs = [CL.source(buf[k].data_ptr(), random_rotation(rng, 0.3), rng.uniform(-0.2, 0.2, 3)) for k in range(n)]   # one room
            cl = CL.Cloud(ctx, rows, cols, n)
            pts, _ = cl.build(srcs, K, args.mode)
            cl.close()
            M = pts.shape[0]
            vox = voxel_total(ctx, pts, args.leaf, args.warmup, args.reps)
            for V in args.views:
                vrng = np.random.default_rng(7 * n + V)
                R = np.stack([random_rotation(vrng, 0.3) for _ in range(V)])
                t = vrng.uniform(-0.2, 0.2, (V, 3))
                rd = RD.Renderer(ctx, M, npix * V)
                for s in args.splats:
                    rd.timing(True)
                    ts = {st: [] for st in RD.STAGES}
                    for k in range(args.warmup + args.reps):
                        planes = rd.render(pts, R, t, K, rows, cols, s, outputs=OUTPUTS)
                        ms = rd.timing(True)
                        if k >= args.warmup:
                            for st, v in ms.items():
                                ts[st].append(v * 1e-3)
                    rd.timing(False)
                    rd.stats(True)
                    rd.render(pts, R, t, K, rows, cols, s, outputs=OUTPUTS)
                    st = rd.stats(False)
                    drawn = int(torch.isfinite(planes["depth"]).sum())
                    med = {k: float(np.median(v)) for k, v in ts.items()}
                    total = sum(med.values())
                    launches = (V + RD.VIEW_CHUNK - 1) // RD.VIEW_CHUNK
                    model = {"clear": 8 * npix * V, "splat": 32 * M * launches,
                             "resolve": (8 + sum(PLANE_BYTES[o] for o in OUTPUTS)) * npix * V + 32 * drawn}
                    line = {"keyframes": n, "mode": args.mode, "points": M, "views": V, "rows": rows, "cols": cols, "splat": s,
                            "stage_us": {k: med[k] * 1e6 for k in RD.STAGES}, "total_us": total * 1e6, "pairs_per_s": M * V / total,
                            "visible_share": st["pairs"] / (M * V), "writes": st["writes"], "atomic_share": st["atomics"] / max(st["writes"], 1),
                            "drawn_share": drawn / (npix * V), "bytes_min": model, "frac_8TBps": {k: model[k] / med[k] / PEAK_BPS for k in RD.STAGES},
                            "voxel_total_us": vox * 1e6, "render_over_voxel": total / vox, "reps": args.reps,
                            "device": torch.cuda.get_device_name(0)}
                    print(json.dumps(line), flush=True)
                    lines.append(line)
                    del planes
                rd.close()
                torch.cuda.empty_cache()
            del pts, buf
            torch.cuda.empty_cache()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
