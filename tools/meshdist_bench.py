#!/usr/bin/env python
"""Point-to-mesh distance throughput (include/rgbid_meshdist.h): analytic sphere states in --sides^3 volumes are extracted, and each mesh is
queried with the vertices of its simplified (cells of 2 voxels) and of its smoothed (5 Taubin iterations) version, in extraction order and
shuffled, with d_max at --dmax voxels and with the handle's query sort on and off.  Each stage is timed with the library's HIP events
(rgbid_meshdist_timing): the median of `reps` plan + query calls after `warmup`; one JSON line per combination, printed and written to
--out, with

    stage_us            the plan's box, pairs, sort and cells stages and the query stage (with its sort when it is on); the host's waits
                        between the plan's stages are not in them
    queries_per_s       queries / the query stage
    candidates          per query, from the `candidates` output: the mean and the largest
    outlier_plan_us     rgbid_outlier's plan over the same points as records at radius d_max in the same process: the one existing pass
                        that walks 27 cells per point, and the only yardstick there is

    python tools/meshdist_bench.py [--sides 256 512] [--dmax 2 8] [--reps 10] [--out profiles/meshdist_bench.jsonl]
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

VOXEL = 0.05


def records_of(points):
    """rgbid_cloud_point records with the positions of float32 [n, 3] and zeros elsewhere"""
    rec = torch.zeros((points.shape[0], 8), dtype=torch.float32, device=points.device)
    rec[:, :3] = points
    return rec.view(torch.uint8).reshape(-1, 32)


def outlier_plan_us(ctx, points, radius, warmup, reps):
    from rgbid import outlier as OL
    rec = records_of(points)
    rf = OL.RadiusFilter(ctx, max(rec.shape[0], 1))
    rf.timing(True)
    total = []
    for k in range(warmup + reps):
        rf.plan(rec, radius, 1, 1 << 31)
        ms = rf.timing(True)
        if k >= warmup:
            total.append(sum(ms.values()) * 1e3)
    rf.close()
    return float(np.median(total))


def measure(ctx, dist, name, mesh, queries, order, voxels, sort, warmup, reps, extra):
    from rgbid import meshdist as MD
    verts, tris = mesh
    dist.sort_queries(sort)
    ts = {st: [] for st in MD.STAGES}
    for k in range(warmup + reps):
        plan = dist.plan(verts, tris, voxels * VOXEL)
        out = dist.query(queries, ("distance", "candidates"))
        ms = dist.timing(True)
        if k >= warmup:
            for st, v in ms.items():
                ts[st].append(v * 1e3)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    cand = out["candidates"].to(torch.int64)
    line = dict(mesh=name, vertices=int(verts.shape[0]), triangles=int(tris.shape[0]), queries=int(queries.shape[0]), order=order, d_max_voxels=voxels,
                d_max_m=voxels * VOXEL, query_sort=bool(sort), plan={k: plan[k] for k in MD.STATS}, stage_us=med,
                plan_us=sum(med[k] for k in MD.STAGES[:4]), queries_per_s=queries.shape[0] / (med["query"] * 1e-6) if med["query"] else None,
                candidates_mean=float(cand.double().mean()) if cand.numel() else 0.0, candidates_max=int(cand.max()) if cand.numel() else 0,
                summary=MD.summary(out["distance"]), reps=reps, library=os.path.relpath(MD._lib.LIB_PATH, ROOT), device=torch.cuda.get_device_name(0))
    line.update(extra)
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--dmax", type=float, nargs="+", default=[2.0, 8.0], help="d_max in voxels")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshdist_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from rgbid import device
    from rgbid import meshdist as MD
    from rgbid import simplify as SP
    from rgbid import smooth as SM
    from rgbid import tsdf as TS
    lines = []
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = device.Context(0)
        for side in args.sides:
            vol = TS.Volume(ctx, side ** 3, 1, colour=False)
            vol.configure(side, side, side, [0.0, 0.0, 0.0], VOXEL, 4 * VOXEL)
            ax = torch.arange(side, dtype=torch.float32, device="cuda") * VOXEL
            c, r = VOXEL * (side - 1) / 2, VOXEL * side * 0.4
            d = torch.sqrt((ax[None, None, :] - c) ** 2 + (ax[None, :, None] - c) ** 2 + (ax[:, None, None] - c) ** 2)
            vol.set_state(torch.clamp(d - r, max=4 * VOXEL).contiguous(), torch.ones((side,) * 3, dtype=torch.int32, device="cuda"))
            del d
            verts, _, tris = vol.extract(1, colours=False)
            vol.close()
            torch.cuda.empty_cache()
            simplified = SP.simplify_mesh(ctx, verts, None, tris, cell=2 * VOXEL)[0]
            smoothed = SM.smooth_mesh(ctx, verts, tris, 5)[0]
            gen = torch.Generator(device="cuda").manual_seed(1)
            for qname, q in (("simplified", simplified), ("smoothed", smoothed)):
                shuffled = q[torch.randperm(q.shape[0], device="cuda", generator=gen)].contiguous()
                for voxels in args.dmax:
                    dist = MD.Distance(ctx, verts.shape[0], tris.shape[0], MD.pair_bound(tris.shape[0], 8), q.shape[0])
                    dist.timing(True)
                    ref = outlier_plan_us(ctx, q, voxels * VOXEL, args.warmup, args.reps)
                    for order, pts in (("extraction", q), ("shuffled", shuffled)):
                        for sort in (True, False):
                            lines.append(measure(ctx, dist, f"sphere {side}^3", (verts, tris), pts, order, voxels, sort, args.warmup, args.reps,
                                                 dict(side=side, voxel_m=VOXEL, query_mesh=qname, outlier_plan_us=ref)))
                    dist.close()
            del verts, tris, simplified, smoothed
            torch.cuda.empty_cache()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
