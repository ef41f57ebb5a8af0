#!/usr/bin/env python
"""Edge-split throughput (include/rgbid_refine.h) on section 32's four meshes: section 22's sphere state in 256^3 (591 062 vertices,
1 182 120 triangles), the same after vertex clustering with a 2-voxel cell, the tracked synthetic run of the tests (24 frames at
160 x 120, a 0.04 m voxel) and the fan of 4 096 triangles around one hub.  max_edge is half the median edge length: one round splits
every edge above it, which cuts most triangles into four and all of them where the edges are of one length.  Each stage is timed with the library's HIP events (rgbid_refine_timing): the median
of `reps` plan + emit calls after `warmup`, positions and triangles only (no colours, normals or selection).  In the same process
rgbid_holes_plan (the same two-round corner sort, then loops where this plan builds an edge table) and one k_smooth_pass are timed on the
same mesh: the yardsticks.  One JSON line per mesh, printed and written to --out, with

    plan_us             check, corner keys, the two sort rounds, the edge scan, the marks and their compaction, k and its scan; the host's
                        wait for the first count is not in it; plan_wall_us is the host clock around the whole synchronising plan call
    emit_us             the word copy of the input's vertices, the new vertices, the triangles
    emit_bytes          24 n_v (the copy) + 44 M (two ends, their two positions, the new row) + 40 n_t (the row, its three edges and their
                        ranks, the base) + 12 (n_t + E) (the rows written): what the contract needs moved once; gathers are counted by
                        their payload, not by the lines they touch
    holes_plan_us, smooth_pass_us   the yardsticks

    python tools/refine_bench.py [--side 256] [--reps 10] [--out profiles/refine_bench.jsonl]
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

from denoise_bench import smooth_pass_us


def median_edge(verts, tris):
    """the median length of the triangles' edges, in float64 on the device"""
    p = verts.double()[tris.long()]
    d = (p - p[:, (1, 2, 0)]).pow(2).sum(2).sqrt().reshape(-1)
    return float(d[torch.isfinite(d)].median().item())


def holes_plan_us(ctx, n_v, tris, warmup, reps):
    from rgbid import holes as HO
    fl = HO.Filler(ctx, max(n_v, 1), max(tris.shape[0], 1))
    fl.timing(True)
    ts = []
    for k in range(warmup + reps):
        fl.plan(tris, n_v)
        ctx.sync()                     # a plan without simple vertices does not wait for its last event
        ms = fl.timing(True)
        if k >= warmup:
            ts.append(ms["plan"] * 1e3)
    fl.close()
    return float(np.median(ts))


def measure(ctx, name, verts, tris, warmup, reps, extra):
    """plan + emit `warmup + reps` times on the mesh, and the yardsticks beside them -> one line"""
    from rgbid import refine as RF
    n_v, n_t = int(verts.shape[0]), int(tris.shape[0])
    max_edge = 0.5 * median_edge(verts, tris)
    rf = RF.Refiner(ctx, max(n_v, 1), max(n_t, 1))
    rf.timing(True)
    ts, wall = {st: [] for st in RF.STAGES}, []
    for k in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        counts = rf.plan(tris, verts, max_edge)
        t1 = time.perf_counter()
        rf.emit(verts, tris)
        ms = rf.timing(True)
        if k >= warmup:
            wall.append(t1 - t0)
            for st, v in ms.items():
                ts[st].append(v * 1e-3)
    rf.close()
    med = {k: float(np.median(v)) for k, v in ts.items()}
    emit_bytes = 24 * n_v + 44 * counts["marked"] + 40 * n_t + 12 * (n_t + counts["new_triangles"])
    line = dict(mesh=name, vertices=n_v, triangles=n_t, max_edge=max_edge, counts=counts, plan_us=med["plan"] * 1e6,
                plan_wall_us=float(np.median(wall)) * 1e6, emit_us=med["emit"] * 1e6, emit_bytes=emit_bytes,
                emit_share_of_8TBps=emit_bytes / med["emit"] / 8e12, holes_plan_us=holes_plan_us(ctx, n_v, tris, warmup, reps),
                smooth_pass_us=smooth_pass_us(ctx, verts, tris, warmup, reps), reps=reps, library=os.path.relpath(RF._lib.LIB_PATH, ROOT),
                device=torch.cuda.get_device_name(0))
    line.update(extra)
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from rgbid import device, sequence, synth
    from rgbid import tsdf as TS
    side, lines = args.side, []
    run = lambda name, v, t, extra: lines.append(measure(ctx, name, v, t, args.warmup, args.reps, extra))
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
        run("sphere", verts, tris, dict(side=side, voxel_m=0.05))
        run("sphere simplified at 2 voxels", sv, st, dict(side=side, voxel_m=0.05))
        del verts, tris, sv, st
        torch.cuda.empty_cache()
        # 2. the tracked run of the tests
        Ks = (synth.TUM_K[0] / 4, synth.TUM_K[1] / 4, (synth.TUM_K[2] + 0.5) / 4 - 0.5, (synth.TUM_K[3] + 0.5) / 4 - 0.5)
        seq = synth.make_sequence(24, K=Ks, rows=120, cols=160, device="cuda", noise=False, dropout=0.0, trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
        depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
        _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, Ks, cloud="novel", visratio_odo=0.985, visratio_integr=0.97, keyframe_depth=True,
                                             keyframe_colour=True)
        verts, _, tris = TS.fuse(ctx, pc.keyframes, Ks, 120, 160, voxel=0.04, points=pc.points)
        run("tracked run", verts, tris, dict(side=None, voxel_m=0.04, keyframes=len(pc.keyframes)))
        # 3. the fan: 4 096 triangles around one hub, whose 4 096 spokes are one run of 8 192 corners in the sort
        fan = np.stack([np.full(4096, 8192), 2 * np.arange(4096), 2 * np.arange(4096) + 1], 1).astype(np.int32)
        pos = np.random.default_rng(2).uniform(-1, 1, (8193, 3)).astype(np.float32)
        run("fan", torch.from_numpy(pos).cuda(), torch.from_numpy(fan).cuda(), dict(side=None, voxel_m=None))
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
