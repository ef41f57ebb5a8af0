#!/usr/bin/env python
"""Vertex recolouring throughput (include/rgbid_recolour.h) on the mesh of the tracked synthetic run of the tests (24 frames at 160 x 120,
fused as tools/raster_bench.py fuses it, with --voxel metres per voxel), coloured from 16 and 64 keyframes of 640 x 480 rendered from the
same scene along the same camera path.  The mesh is rasterised at the keyframes' poses (depth only) and recoloured with those planes as
`surface`, once without and once with the keyframes' own inverse depth, with the mesh's normals.  Each stage is timed with the libraries'
HIP events (rgbid_recolour_timing, rgbid_raster_timing): the median of `reps` calls after `warmup`; one JSON line per configuration,
printed and written to --out, with

    accumulate_us, resolve_us      the two stages of the recolouring (all launches of one add; one finish)
    raster_us                      the rasteriser's four stages for the same views in the same run
    accumulate_over_raster         which half of recolour_mesh costs more
    ns_per_vertex_view             accumulate over vertices x views
    contract_bytes                 what the contract makes the kernel touch: per TAKEN pair 12 colour bytes and 16 per optional plane, and
                                   per vertex and launch of 16 views the state read and written (72), the position and the normal (24)
    roofline_share                 contract_bytes over accumulate, over 8 TB/s

    python tools/recolour_bench.py [--voxel 0.01] [--reps 10] [--out profiles/recolour_bench.jsonl]
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

ROWS, COLS = 480, 640
HBM_BYTES_PER_S = 8e12


def measure(ctx, verts, tris, normals, kfs, Kc, measured, mode, warmup, reps, extra):
    from rgbid import raster as RS
    from rgbid import recolour as RC
    V, n_v = len(kfs), verts.shape[0]
    R, t = np.stack([k["R"] for k in kfs]), np.stack([k["t"] for k in kfs])
    rs = RS.Rasteriser(ctx, n_v, tris.shape[0], ROWS * COLS * V)
    rc = RC.Recolourer(ctx, n_v)
    rs.timing(True); rc.timing(True)
    ts = dict(raster=[], accumulate=[], resolve=[])
    for k in range(warmup + reps):
        depth = rs.render(verts, tris, R, t, Kc, ROWS, COLS, None, None, outputs=("depth",))["depth"]
        raster_ms = sum(rs.timing(True).values())
        rc.begin(n_v, mode)
        rc.add(verts, R, t, Kc, ROWS, COLS, [k_["colour"] for k_ in kfs], depth, [k_["depthinv"] for k_ in kfs] if measured else None, normals,
               surface_tolerance=extra["surface_tolerance_m"], measured_tolerance=extra["surface_tolerance_m"])
        out = rc.finish()
        ms = rc.timing(True)
        if k >= warmup:
            ts["raster"].append(raster_ms * 1e3); ts["accumulate"].append(ms["accumulate"] * 1e3); ts["resolve"].append(ms["resolve"] * 1e3)
    counts = RC.counts_total(rc.counts())
    rc.close(); rs.close()
    med = {k: float(np.median(v)) for k, v in ts.items()}
    launches = (V + RC.VIEW_CHUNK - 1) // RC.VIEW_CHUNK
    per_pair = 12 + 16 * (2 if measured else 1)
    contract = counts["taken"] * per_pair + n_v * launches * (72 + 24)
    line = dict(mesh="tracked run", vertices=int(n_v), triangles=int(tris.shape[0]), views=V, rows=ROWS, cols=COLS, mode=mode, planes=["surface"] + (["depthinv"] if measured else []),
                normals=normals is not None, counts=counts, coloured=int((out["views_used"] != 0).sum()), accumulate_us=med["accumulate"], accumulate_us_range=[min(ts["accumulate"]), max(ts["accumulate"])],
                resolve_us=med["resolve"],
                raster_us=med["raster"], accumulate_over_raster=med["accumulate"] / med["raster"], ns_per_vertex_view=med["accumulate"] * 1e3 / (n_v * V),
                bytes_per_taken_pair=per_pair, contract_bytes=int(contract), roofline_share=contract / (med["accumulate"] * 1e-6) / HBM_BYTES_PER_S, reps=reps,
                library=os.path.relpath(RC._lib.LIB_PATH, ROOT), device=torch.cuda.get_device_name(0))
    line.update(extra)
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--views", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recolour_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from rgbid import device, sequence, synth
    from rgbid import tsdf as TS
    lines = []
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = device.Context(0)
        Ks = (synth.TUM_K[0] / 4, synth.TUM_K[1] / 4, (synth.TUM_K[2] + 0.5) / 4 - 0.5, (synth.TUM_K[3] + 0.5) / 4 - 0.5)
        path = dict(trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
        seq = synth.make_sequence(24, K=Ks, rows=120, cols=160, device="cuda", noise=False, dropout=0.0, **path)
        depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
        _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, Ks, cloud="novel", visratio_odo=0.985, visratio_integr=0.97, keyframe_depth=True,
                                             keyframe_colour=True)
        voxel = args.voxel
        while True:
            try:
                verts, _, tris, normals = TS.fuse(ctx, pc.keyframes, Ks, 120, 160, voxel=voxel, points=pc.points, normals=True)
                break
            except ValueError as e:                         # more voxels than fuse allocates: say so and take a coarser grid
                print(f"voxel {voxel:g} m: {e}; doubling it", flush=True)
                voxel *= 2
        for V in args.views:
            full = synth.make_sequence(V, K=tuple(synth.TUM_K), rows=ROWS, cols=COLS, device="cuda", noise=False, dropout=0.0, **path)
            d = full["depth"].to(torch.float32)
            iD = torch.where(d > 0, 1000.0 / d, torch.zeros_like(d))
            kfs = [dict(R=full["R_wc"][k].cpu().numpy(), t=full["t_wc"][k].cpu().numpy(), depthinv=iD[k].contiguous(), colour=full["rgb"][k].contiguous())
                   for k in range(V)]
            extra = dict(voxel_m=voxel, surface_tolerance_m=2 * voxel)
            for measured in (False, True):
                lines.append(measure(ctx, verts, tris, normals, kfs, tuple(synth.TUM_K), measured, "mean", args.warmup, args.reps, extra))
            lines.append(measure(ctx, verts, tris, normals, kfs, tuple(synth.TUM_K), True, "best", args.warmup, args.reps, extra))
            del full, d, iD, kfs
            torch.cuda.empty_cache()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
