#!/usr/bin/env python
"""Texture-atlas throughput (include/rgbid_texture.h) on the mesh of tools/recolour_bench.py (the tracked synthetic run of the tests, 24
frames at 160 x 120, fused at --voxel metres per voxel) simplified at --simplify metres, textured at patch 6 and 14 from 16 and 64
keyframes of 640 x 480 rendered from the same scene along the same camera path.  The mesh is rasterised at the keyframes' poses (depth
only) and textured with those planes as `surface` and the mesh's normals.  Accumulate and resolve are timed with the library's HIP events
(rgbid_texture_timing): the median of `reps` calls after `warmup`; one JSON line per configuration, printed and appended to --out, with

    accumulate_us, resolve_us      all launches of one add; one finish
    ns_per_texel_view              accumulate over used texels x views (section 27 measured 0.0176 - 0.0235 ns per vertex x view)
    contract_bytes                 what the contract makes the kernel touch: per TAKEN pair 12 colour bytes and 16 per plane, per used texel
                                   and launch of 16 views the state read and written (72), per triangle and launch its indices, corners and
                                   normals (84)
    roofline_share                 contract_bytes over accumulate, over 8 TB/s

    python tools/texture_bench.py [--voxel 0.01] [--simplify 0.04] [--reps 10] [--out profiles/texture_bench.jsonl]
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


def measure(ctx, verts, tris, normals, kfs, Kc, patch, mode, warmup, reps, extra):
    from rgbid import raster as RS
    from rgbid import recolour as RC
    from rgbid import texture as TX
    V, n_v, n_t = len(kfs), verts.shape[0], tris.shape[0]
    R, t = np.stack([k["R"] for k in kfs]), np.stack([k["t"] for k in kfs])
    lay = TX.layout(n_t, patch)
    rs = RS.Rasteriser(ctx, n_v, n_t, ROWS * COLS * V)
    tx = TX.Texturer(ctx, n_t, lay["slots"])
    tx.timing(True)
    depth = rs.render(verts, tris, R, t, Kc, ROWS, COLS, None, None, outputs=("depth",))["depth"]
    ts = dict(accumulate=[], resolve=[])
    for k in range(warmup + reps):
        tx.begin(n_t, patch, lay["tiles_x"], mode)
        tx.add(verts, tris, R, t, Kc, ROWS, COLS, [k_["colour"] for k_ in kfs], depth, None, normals, surface_tolerance=extra["surface_tolerance_m"])
        out = tx.finish()
        ms = tx.timing(True)
        if k >= warmup:
            ts["accumulate"].append(ms["accumulate"] * 1e3); ts["resolve"].append(ms["resolve"] * 1e3)
    counts = RC.counts_total(tx.counts())
    tx.close(); rs.close()
    med = {k: float(np.median(v)) for k, v in ts.items()}
    texels = n_t * lay["texels_per_triangle"]
    launches = (V + RC.VIEW_CHUNK - 1) // RC.VIEW_CHUNK
    per_pair = 12 + 16
    contract = counts["taken"] * per_pair + launches * (texels * 72 + n_t * 84)
    line = dict(mesh="tracked run, simplified", vertices=int(n_v), triangles=int(n_t), patch=patch, atlas=[lay["W"], lay["H"]], slots=lay["slots"], texels=texels,
                views=V, rows=ROWS, cols=COLS, mode=mode, planes=["surface"], normals=True, counts=counts, textured=int((out["views_used"] != 0).sum()),
                accumulate_us=med["accumulate"], accumulate_us_range=[min(ts["accumulate"]), max(ts["accumulate"])], resolve_us=med["resolve"],
                resolve_us_range=[min(ts["resolve"]), max(ts["resolve"])], ns_per_texel_view=med["accumulate"] * 1e3 / max(texels * V, 1),
                bytes_per_taken_pair=per_pair, contract_bytes=int(contract), roofline_share=contract / (med["accumulate"] * 1e-6) / HBM_BYTES_PER_S, reps=reps,
                library=os.path.relpath(TX._lib.LIB_PATH, ROOT), device=torch.cuda.get_device_name(0))
    line.update(extra)
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--simplify", type=float, default=0.04)
    ap.add_argument("--views", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--patch", type=int, nargs="+", default=[6, 14])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_bench.jsonl"))
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
                verts, _, tris, normals = TS.fuse(ctx, pc.keyframes, Ks, 120, 160, voxel=voxel, points=pc.points, normals=True, simplify=args.simplify)
                break
            except ValueError as e:                         # more voxels than fuse allocates: say so and take a coarser grid
                print(f"voxel {voxel:g} m: {e}; doubling it", flush=True)
                voxel *= 2
        for V in args.views:
            full = synth.make_sequence(V, K=tuple(synth.TUM_K), rows=ROWS, cols=COLS, device="cuda", noise=False, dropout=0.0, **path)
            kfs = [dict(R=full["R_wc"][k].cpu().numpy(), t=full["t_wc"][k].cpu().numpy(), colour=full["rgb"][k].contiguous()) for k in range(V)]
            extra = dict(voxel_m=voxel, simplify_m=args.simplify, surface_tolerance_m=2 * voxel)
            for patch in args.patch:
                for mode in ("mean", "best"):
                    lines.append(measure(ctx, verts, tris, normals, kfs, tuple(synth.TUM_K), patch, mode, args.warmup, args.reps, extra))
            del full, kfs
            torch.cuda.empty_cache()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
