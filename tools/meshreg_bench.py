#!/usr/bin/env python
"""Registration cost per iteration (include/rgbid_meshreg.h): section 26's analytic sphere in a --sides^3 volume is extracted, and the
vertices of its smoothed version (5 Taubin iterations), moved rigidly by 0.02 rad and half a voxel, are registered back to it from
--starts perturbed starts at once, with d_max at --dmax voxels, over one level of every point and --iterations iterations whose eps no
step meets, so that every iteration runs.  Each stage is timed with the library's HIP events (rgbid_meshreg_timing), summed over the
iterations of a call: the median of `reps` calls after `warmup`; one JSON line per combination, printed and written to --out, with

    stage_us_per_iteration   transform, query (the truncated nearest-triangle search with its sort), system, solve
    launches_per_iteration   what one iteration enqueues, counted from the source: the search's own launches depend on its sort
    iterations               systems built by the slowest start (all of them, unless a start stopped)

    python tools/meshreg_bench.py [--sides 256] [--dmax 2 8] [--starts 1 4] [--iterations 10] [--reps 10] [--out profiles/meshreg_bench.jsonl]
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


def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def measure(reg, name, points, R, t, voxels, iterations, sort, warmup, reps, extra):
    from rgbid import meshreg as MR
    reg.sort_queries(sort)
    levels = ((1, iterations, voxels * VOXEL),)
    ts = {st: [] for st in MR.STAGES}
    for k in range(warmup + reps):
        res = reg.align(points, R, t, levels=levels, eps=1e-300)
        ms = reg.timing(True)
        if k >= warmup:
            for st, v in ms.items():
                ts[st].append(v * 1e3)
    its = int(res["iterations"].max())
    med = {k: float(np.median(v)) / its for k, v in ts.items()}
    line = dict(mesh=name, points=int(points.shape[0]), starts=len(R), d_max_voxels=voxels, d_max_m=voxels * VOXEL, query_sort=bool(sort), iterations=its,
                status=[MR.STATUS[int(s)] for s in res["status"]], used=[int(u) for u in res["used"][:, 1]], rms_m=[float(x) for x in MR.rms(res)],
                stage_us_per_iteration=med, iteration_us=sum(med.values()), launches_per_iteration="transform 1 + query (sort on: keys and sort passes, + 1) + system 1 + solve 1",
                reps=reps, device=torch.cuda.get_device_name(0))
    line.update(extra)
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[256])
    ap.add_argument("--dmax", type=float, nargs="+", default=[2.0, 8.0], help="d_max in voxels")
    ap.add_argument("--starts", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshreg_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from rgbid import device
    from rgbid import meshdist as MD
    from rgbid import meshreg as MR
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
            smoothed = SM.smooth_mesh(ctx, verts, tris, 5)[0]
            centre = np.full(3, c)
            Rm = rotation((1, 2, 3), 0.02)
            tm = centre - Rm @ centre + np.array([0.5, -0.3, 0.2]) * VOXEL
            mover = MR.Registration(ctx, 1, 1, 1, 1, 1)
            moved = mover.apply(smoothed, Rm.T, -Rm.T @ tm)      # (Rm, tm) brings it back
            mover.close()
            for voxels in args.dmax:
                for V in args.starts:
                    rng = np.random.default_rng(V)
                    R = np.stack([rotation(rng.normal(size=3), 0.005 * k) @ Rm for k in range(V)])
                    t = np.stack([centre - R[k] @ (Rm.T @ (centre - tm)) for k in range(V)])
                    reg = MR.Registration(ctx, verts.shape[0], tris.shape[0], MD.pair_bound(tris.shape[0], 8), moved.shape[0], V)
                    reg.target(verts, tris, voxels * VOXEL)
                    reg.timing(True)
                    for sort in (True, False):
                        lines.append(measure(reg, f"sphere {side}^3", moved, R, t, voxels, args.iterations, sort, args.warmup, args.reps,
                                             dict(side=side, voxel_m=VOXEL, vertices=int(verts.shape[0]), triangles=int(tris.shape[0]))))
                    reg.close()
            del verts, tris, smoothed, moved
            torch.cuda.empty_cache()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
