#!/usr/bin/env python
"""Vertex clustering throughput (include/rgbid_simplify.h) on two meshes: section 22's sphere state in 256^3 (591 062 vertices, 1 182 120
triangles, one closed component) and the tracked synthetic run of the tests (24 frames at 160 x 120, a 0.04 m voxel).  Each stage is timed
with the library's HIP events (rgbid_simplify_timing): the median of `reps` plan + emit calls after `warmup`; one JSON line per mesh, cell
and duplicate mode, printed and written to --out, with

    stage_us            vertices (box, keys, sort, runs and cluster map), triangles (classes, the three sort rounds, heads, count), emit
                        (representatives, cluster_of, the kept triangles).  The host's waits between the plan's stages are not in them;
                        plan_wall_us is the host clock around the whole synchronising plan call
    counts              what the plan found: participating, clusters, lost, collapsed, duplicate, kept

    python tools/simplify_bench.py [--side 256] [--cells 2 4 8] [--reps 10] [--out profiles/simplify_bench.jsonl]
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


def measure(ctx, name, mesh, voxel, factor, keep_duplicates, warmup, reps, extra):
    """plan + emit `warmup + reps` times on the mesh (vertices, colours, triangles, normals) with a cell of factor x voxel -> one line"""
    from rgbid import simplify as SP
    verts, cols, tris, nrm = mesh
    sp = SP.Simplifier(ctx, max(verts.shape[0], 1), max(tris.shape[0], 1))
    sp.timing(True)
    ts, wall = {st: [] for st in SP.STAGES}, []
    for k in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        plan = sp.plan(verts, tris, factor * voxel, keep_duplicates)
        t1 = time.perf_counter()
        sp.emit(cols, nrm)
        ms = sp.timing(True)
        if k >= warmup:
            wall.append(t1 - t0)
            for st, v in ms.items():
                ts[st].append(v * 1e-3)
    sp.close()
    med = {k: float(np.median(v)) for k, v in ts.items()}
    line = dict(mesh=name, vertices=int(verts.shape[0]), triangles=int(tris.shape[0]), cell_m=factor * voxel, cell_voxels=factor,
                keep_duplicates=keep_duplicates, counts={k: plan[k] for k in SP.COUNTS}, stage_us={k: med[k] * 1e6 for k in SP.STAGES},
                total_us=sum(med.values()) * 1e6, plan_wall_us=float(np.median(wall)) * 1e6, reps=reps,
                library=os.path.relpath(SP._lib.LIB_PATH, ROOT), device=torch.cuda.get_device_name(0))
    line.update(extra)
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0, 8.0], help="cell edges in voxels")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from rgbid import device, sequence, synth
    from rgbid import tsdf as TS
    side, lines = args.side, []
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = device.Context(0)
        # 1. section 22's sphere: one closed component
        vol = TS.Volume(ctx, side ** 3, 1)
        vol.configure(side, side, side, [0.0, 0.0, 0.0], 0.05, 0.2)
        ax = torch.arange(side, dtype=torch.float32, device="cuda") * 0.05
        c, r = 0.05 * (side - 1) / 2, 0.05 * side * 0.4
        dist = torch.sqrt((ax[None, None, :] - c) ** 2 + (ax[None, :, None] - c) ** 2 + (ax[:, None, None] - c) ** 2)
        vol.set_state(torch.clamp(dist - r, max=0.2).contiguous(), torch.ones((side,) * 3, dtype=torch.int32, device="cuda"))
        del dist
        mesh = vol.extract(1, normals=True)
        vol.close()
        for factor in args.cells:
            for keep in (False, True):
                lines.append(measure(ctx, "sphere", mesh, 0.05, factor, keep, args.warmup, args.reps, dict(side=side, voxel_m=0.05)))
        del mesh
        torch.cuda.empty_cache()
        # 2. the tracked run of the tests
        Ks = (synth.TUM_K[0] / 4, synth.TUM_K[1] / 4, (synth.TUM_K[2] + 0.5) / 4 - 0.5, (synth.TUM_K[3] + 0.5) / 4 - 0.5)
        seq = synth.make_sequence(24, K=Ks, rows=120, cols=160, device="cuda", noise=False, dropout=0.0, trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
        depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
        _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, Ks, cloud="novel", visratio_odo=0.985, visratio_integr=0.97, keyframe_depth=True,
                                             keyframe_colour=True)
        mesh = TS.fuse(ctx, pc.keyframes, Ks, 120, 160, voxel=0.04, points=pc.points, normals=True)
        lines.append(measure(ctx, "tracked run", mesh, 0.04, 2.0, False, args.warmup, args.reps, dict(side=None, voxel_m=0.04, keyframes=len(pc.keyframes))))
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
