#!/usr/bin/env python
"""Hole filling throughput (include/rgbid_holes.h) on three meshes: section 22's sphere state in 256^3 (591 062 vertices, 1 182 120
triangles) without the triangles of every 40th vertex, the same after vertex clustering with a 2-voxel cell, and the tracked synthetic run
of the tests (24 frames at 160 x 120, a 0.04 m voxel).  Each stage is timed with the library's HIP events (rgbid_holes_timing): the median
of `reps` plan + select + emit calls after `warmup`.  In the same process rgbid_smooth_plan is timed on the same mesh: the one existing
pass with the same two-round sort over the triangles (its pairs are twice the corners, and it builds a CSR where this plan builds loops),
and the only yardstick.  One JSON line per mesh, printed and written to --out, with

    plan_us             check, corner keys, the two sort rounds, compaction, degrees, the simple vertices, 2 x `rounds` doubling launches,
                        the loop table; the host's wait for the first count is not in it, the wait for the number of simple vertices is;
                        plan_wall_us is the host clock around the whole synchronising plan call
    select_us           the walk of every loop, the ranks and the bases
    emit_us             the word copies of the inputs, the fans, the new vertices with colours and normals
    smooth_plan_us      rgbid_smooth_plan without normals on the same triangles, and its wall clock

    python tools/holes_bench.py [--side 256] [--max-edges 64] [--reps 10] [--out profiles/holes_bench.jsonl]
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


def punched(tris, every):
    """the triangles that name no vertex whose index is a multiple of `every`"""
    return tris[((tris % every) != 0).all(1)].contiguous()


def measure(ctx, name, verts, cols, tris, nrm, max_edges, warmup, reps, extra):
    """plan + select + emit `warmup + reps` times on the mesh, and the smoothing plan beside them -> one line"""
    from rgbid import holes as HO
    from rgbid import smooth as SO
    n_v, n_t = int(verts.shape[0]), int(tris.shape[0])
    fl = HO.Filler(ctx, max(n_v, 1), max(n_t, 1))
    sm = SO.Smoother(ctx, max(n_v, 1), max(n_t, 1))
    fl.timing(True)
    sm.timing(True)
    ts, wall, smooth, smooth_wall = {st: [] for st in HO.STAGES}, [], [], []
    for k in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        plan = fl.plan(tris, n_v)
        t1 = time.perf_counter()
        chosen = fl.select(verts, max_edges)
        fl.emit(verts, tris, cols, nrm)
        ms = fl.timing(True)
        ctx.sync()
        t2 = time.perf_counter()
        sm.plan(tris, n_v)
        t3 = time.perf_counter()
        sms = sm.timing(True)
        if k >= warmup:
            wall.append(t1 - t0)
            smooth_wall.append(t3 - t2)
            smooth.append(sms["plan"] * 1e-3)
            for st, v in ms.items():
                ts[st].append(v * 1e-3)
    fl.close()
    sm.close()
    med = {k: float(np.median(v)) for k, v in ts.items()}
    simple = plan["boundary_vertices"] - plan["non_simple"]
    line = dict(mesh=name, vertices=n_v, triangles=n_t, max_edges=max_edges, counts=dict(plan, **chosen), simple_vertices=simple,
                rounds=int(simple).bit_length(), plan_us=med["plan"] * 1e6, select_us=med["select"] * 1e6, emit_us=med["emit"] * 1e6,
                plan_wall_us=float(np.median(wall)) * 1e6, smooth_plan_us=float(np.median(smooth)) * 1e6,
                smooth_plan_wall_us=float(np.median(smooth_wall)) * 1e6, reps=reps, library=os.path.relpath(HO._lib.LIB_PATH, ROOT),
                device=torch.cuda.get_device_name(0))
    line.update(extra)
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--max-edges", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "holes_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from rgbid import device, sequence, synth
    from rgbid import tsdf as TS
    side, lines = args.side, []
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = device.Context(0)
        # 1. section 22's sphere without the triangles of every 40th vertex, and the same after vertex clustering at 2 voxels
        vol = TS.Volume(ctx, side ** 3, 1)
        vol.configure(side, side, side, [0.0, 0.0, 0.0], 0.05, 0.2)
        ax = torch.arange(side, dtype=torch.float32, device="cuda") * 0.05
        c, r = 0.05 * (side - 1) / 2, 0.05 * side * 0.4
        dist = torch.sqrt((ax[None, None, :] - c) ** 2 + (ax[None, :, None] - c) ** 2 + (ax[:, None, None] - c) ** 2)
        vol.set_state(torch.clamp(dist - r, max=0.2).contiguous(), torch.ones((side,) * 3, dtype=torch.int32, device="cuda"))
        del dist
        verts, _, tris, nrm = vol.extract(1, colours=False, normals=True)
        sv, _, st, sn = vol.extract(1, colours=False, normals=True, simplify=0.1)
        vol.close()
        lines.append(measure(ctx, "sphere punched at every 40th vertex", verts, None, punched(tris, 40), nrm, args.max_edges, args.warmup, args.reps,
                             dict(side=side, voxel_m=0.05)))
        lines.append(measure(ctx, "sphere simplified at 2 voxels, punched", sv, None, punched(st, 40), sn, args.max_edges, args.warmup, args.reps,
                             dict(side=side, voxel_m=0.05)))
        del verts, tris, nrm, sv, st, sn
        torch.cuda.empty_cache()
        # 2. the tracked run of the tests
        Ks = (synth.TUM_K[0] / 4, synth.TUM_K[1] / 4, (synth.TUM_K[2] + 0.5) / 4 - 0.5, (synth.TUM_K[3] + 0.5) / 4 - 0.5)
        seq = synth.make_sequence(24, K=Ks, rows=120, cols=160, device="cuda", noise=False, dropout=0.0, trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
        depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
        _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, Ks, cloud="novel", visratio_odo=0.985, visratio_integr=0.97, keyframe_depth=True,
                                             keyframe_colour=True)
        verts, cols, tris, nrm = TS.fuse(ctx, pc.keyframes, Ks, 120, 160, voxel=0.04, points=pc.points, normals=True)
        lines.append(measure(ctx, "tracked run", verts, cols, tris, nrm, args.max_edges, args.warmup, args.reps,
                             dict(side=None, voxel_m=0.04, keyframes=len(pc.keyframes))))
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
