#!/usr/bin/env python
"""Taubin smoothing throughput (include/rgbid_smooth.h) on four meshes: section 22's sphere state in 256^3 (591 062 vertices, 1 182 120
triangles, one closed component), the same sphere after vertex clustering with a 2-voxel cell, the tracked synthetic run of the tests (24
frames at 160 x 120, a 0.04 m voxel) and section 22's fan of 4 096 triangles, whose hub's row is walked by one thread: the serial worst
case.  Each stage is timed with the library's HIP events (rgbid_smooth_timing): the median of `reps` plan + run + normals calls after
`warmup`; one JSON line per mesh, printed and written to --out, with

    plan_us             check, pair keys, the two sort rounds, compaction, rows, offsets, boundary bytes, the corner table; the host's wait
                        for the first count is not in it; plan_wall_us is the host clock around the whole synchronising plan call
    pass_us             run_us / passes: `iterations` iterations are 2 x iterations passes, enqueued without a host wait
    normals_us          the normals kernel over the smoothed positions
    pass_bytes          what one pass must move, 24 n_v + 4 P + 4 (n_v + 1), and pass_share_of_8TBps, those bytes over pass_us against 8 TB/s

    python tools/smooth_bench.py [--side 256] [--iterations 10] [--reps 10] [--out profiles/smooth_bench.jsonl]
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


def measure(ctx, name, verts, tris, iterations, warmup, reps, extra):
    """plan + run + normals `warmup + reps` times on the mesh -> one line"""
    from rgbid import smooth as SO
    sm = SO.Smoother(ctx, max(verts.shape[0], 1), max(tris.shape[0], 1))
    sm.timing(True)
    ts, wall = {st: [] for st in SO.STAGES}, []
    for k in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        plan = sm.plan(tris, verts.shape[0], normals=True)
        t1 = time.perf_counter()
        out = sm.run(verts, iterations)
        sm.normals(out)
        ms = sm.timing(True)
        if k >= warmup:
            wall.append(t1 - t0)
            for st, v in ms.items():
                ts[st].append(v * 1e-3)
    sm.close()
    med = {k: float(np.median(v)) for k, v in ts.items()}
    n_v, passes = int(verts.shape[0]), 2 * iterations
    pass_bytes = 24 * n_v + 4 * plan["pairs"] + 4 * (n_v + 1)
    pass_us = med["run"] * 1e6 / passes
    line = dict(mesh=name, vertices=n_v, triangles=int(tris.shape[0]), iterations=iterations, passes=passes, counts=plan, plan_us=med["plan"] * 1e6,
                run_us=med["run"] * 1e6, pass_us=pass_us, normals_us=med["normals"] * 1e6, plan_wall_us=float(np.median(wall)) * 1e6,
                pass_bytes=pass_bytes, pass_share_of_8TBps=pass_bytes / (pass_us * 1e-6) / 8e12, reps=reps,
                library=os.path.relpath(SO._lib.LIB_PATH, ROOT), device=torch.cuda.get_device_name(0))
    line.update(extra)
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from rgbid import device, sequence, synth
    from rgbid import tsdf as TS
    side, lines = args.side, []
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = device.Context(0)
        # 1. section 22's sphere: one closed component, and what vertex clustering at 2 voxels leaves of it
        vol = TS.Volume(ctx, side ** 3, 1)
        vol.configure(side, side, side, [0.0, 0.0, 0.0], 0.05, 0.2)
        ax = torch.arange(side, dtype=torch.float32, device="cuda") * 0.05
        c, r = 0.05 * (side - 1) / 2, 0.05 * side * 0.4
        dist = torch.sqrt((ax[None, None, :] - c) ** 2 + (ax[None, :, None] - c) ** 2 + (ax[:, None, None] - c) ** 2)
        vol.set_state(torch.clamp(dist - r, max=0.2).contiguous(), torch.ones((side,) * 3, dtype=torch.int32, device="cuda"))
        del dist
        verts, _, tris = vol.extract(1, colours=False)
        sv, _, st = vol.extract(1, colours=False, simplify=0.1)
        vol.close()
        lines.append(measure(ctx, "sphere", verts, tris, args.iterations, args.warmup, args.reps, dict(side=side, voxel_m=0.05)))
        lines.append(measure(ctx, "sphere simplified at 2 voxels", sv, st, args.iterations, args.warmup, args.reps, dict(side=side, voxel_m=0.05)))
        del verts, tris, sv, st
        torch.cuda.empty_cache()
        # 2. the tracked run of the tests
        Ks = (synth.TUM_K[0] / 4, synth.TUM_K[1] / 4, (synth.TUM_K[2] + 0.5) / 4 - 0.5, (synth.TUM_K[3] + 0.5) / 4 - 0.5)
        seq = synth.make_sequence(24, K=Ks, rows=120, cols=160, device="cuda", noise=False, dropout=0.0, trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
        depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
        _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, Ks, cloud="novel", visratio_odo=0.985, visratio_integr=0.97, keyframe_depth=True,
                                             keyframe_colour=True)
        verts, _, tris = TS.fuse(ctx, pc.keyframes, Ks, 120, 160, voxel=0.04, points=pc.points)
        lines.append(measure(ctx, "tracked run", verts, tris, args.iterations, args.warmup, args.reps, dict(side=None, voxel_m=0.04, keyframes=len(pc.keyframes))))
        # 3. the fan: 4 096 triangles around one hub, whose row of 8 192 neighbours one thread walks
        fan = np.stack([np.full(4096, 8192), 2 * np.arange(4096), 2 * np.arange(4096) + 1], 1).astype(np.int32)
        pos = np.random.default_rng(2).uniform(-1, 1, (8193, 3)).astype(np.float32)
        lines.append(measure(ctx, "fan", torch.from_numpy(pos).cuda(), torch.from_numpy(fan).cuda(), args.iterations, args.warmup, args.reps,
                             dict(side=None, voxel_m=None)))
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
