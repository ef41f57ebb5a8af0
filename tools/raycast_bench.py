#!/usr/bin/env python
"""TSDF ray-cast and vertex-normal throughput (include/rgbid_tsdf_raycast.h) on the volumes of tools/tsdf_bench.py: the batch's keyframes
(n synthesised 640 x 480 export blocks with random poses near the origin, one room) are integrated into a cube of `side`^3 voxels over the
box of the batch's cloud, and the volume is ray-cast at the keyframes' own poses with step = voxel.  The ray cast is timed with the
library's HIP events (rgbid_tsdf_raycast_timing): the median of `reps` calls after `warmup`; one JSON line per (batch, side), printed and
written to --out, with

    raycast_us          the pose table's upload and the launch, all three planes written
    rays_per_s          views x rows x cols over that time
    hits                pixels with a depth
    emit_call_us,       a host clock around rgbid_tsdf_extract_emit and around rgbid_tsdf_extract_normals, each ended by a stream
    normals_call_us     synchronise (the library times no normal stage of its own): the vertex-normal write beside the mesh write
    render_us           rgbid_render of the same batch's cloud at the same poses with splat 1, in the same process (clear + splat +
                        resolve, its own HIP events): the one existing pass that produces these planes.  Nothing about the ratio is
                        asserted: the synthetic batches' surface is noise, the worst case for the march

    python tools/raycast_bench.py [--sizes 16] [--sides 256 512] [--reps 10] [--out profiles/raycast_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rgbid-slam_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch


def render_time(ctx, pts, R, t, K, rows, cols, warmup, reps):
    """median seconds of the cloud renderer's three stages over pts at the given poses, splat 1"""
    from rgbid import render as RD
    rd = RD.Renderer(ctx, pts.shape[0], rows * cols * len(R))
    rd.timing(True)
    ts = []
    for k in range(warmup + reps):
        rd.render(pts, R, t, K, rows, cols, 1, outputs=("depth", "colour", "normal"))
        ms = rd.timing(True)
        if k >= warmup:
            ts.append(sum(ms.values()) * 1e-3)
    rd.close()
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16])
    ap.add_argument("--sides", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--mode", choices=["novel", "all"], default="novel")
    ap.add_argument("--trunc-voxels", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast_bench.jsonl"))
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
            R = np.stack([random_rotation(rng, 0.3) for _ in range(n)])       # one room: the batch of tools/tsdf_bench.py
            t = rng.uniform(-0.2, 0.2, (n, 3))
            cl = CL.Cloud(ctx, rows, cols, n)
            pts, offsets = cl.build([CL.source(buf[k].data_ptr(), R[k], t[k]) for k in range(n)], K, args.mode)
            cl.close()
            planes = [buf[k, 4 * N:8 * N].view(torch.float32).view(rows, cols) for k in range(n)]
            colours = [buf[k, N:4 * N].view(rows, cols, 3) for k in range(n)]
            render = render_time(ctx, pts, R, t, K, rows, cols, args.warmup, args.reps)
            box = np.array(TS.cloud_bounds(pts))
            for side in args.sides:
                voxel = float((box[3:] - box[:3]).max() / (side - 1))
                vol = TS.Volume(ctx, side ** 3, n)
                vol.configure(side, side, side, [float(v) for v in box[:3]], voxel, args.trunc_voxels * voxel)
                vol.integrate(planes, colours, R, t, K, rows, cols)
                vol.raycast_timing(True)
                ts, out = [], None
                for k in range(args.warmup + args.reps):
                    out = vol.raycast(R, t, K, rows, cols)                     # step = voxel
                    ms = vol.raycast_timing(True)
                    if k >= args.warmup:
                        ts.append(ms * 1e-3)
                vol.raycast_timing(False)
                hits = int(torch.isfinite(out["depth"]).sum().item())
                verts, vcols, tris = vol.extract(1)                            # leaves the plan
                nrm = torch.empty_like(verts)
                te, tn = [], []
                for k in range(args.warmup + args.reps):
                    ctx.wait_torch_stream(); ctx.sync()
                    t0 = time.perf_counter(); vol.emit(verts, vcols, tris); ctx.sync(); t1 = time.perf_counter()
                    vol.emit_normals(nrm); ctx.sync(); t2 = time.perf_counter()
                    if k >= args.warmup:
                        te.append(t1 - t0); tn.append(t2 - t1)
                vol.close()
                cast = float(np.median(ts))
                line = {"keyframes": n, "mode": args.mode, "views": n, "rows": rows, "cols": cols, "side": side, "voxels": side ** 3, "voxel_m": voxel,
                        "step_m": voxel, "raycast_us": cast * 1e6, "rays_per_s": n * N / cast, "hits": hits, "vertices": int(verts.shape[0]),
                        "triangles": int(tris.shape[0]), "emit_call_us": float(np.median(te)) * 1e6, "normals_call_us": float(np.median(tn)) * 1e6,
                        "points": int(pts.shape[0]), "render_us": render * 1e6, "raycast_over_render": cast / render, "reps": args.reps,
                        "library": os.path.relpath(TS._lib.LIB_PATH, ROOT), "device": torch.cuda.get_device_name(0)}
                print(json.dumps(line), flush=True)
                lines.append(line)
                del verts, vcols, tris, nrm, out
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
