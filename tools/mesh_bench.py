#!/usr/bin/env python
"""Mesh component filter throughput (include/rgbid_mesh.h) on three meshes: the 256^3 mesh of the 16-block batch of tools/tsdf_bench.py
(synthesised export blocks with random poses: shards, so many components), a synthetic sphere state in 256^3 (one component) and the
tracked synthetic run of the tests (24 frames at 160 x 120, a 0.04 m voxel).  Each stage is timed with the library's HIP events
(rgbid_mesh_timing): the median of `reps` label + select + emit calls after `warmup`; one JSON line per mesh, printed and written to --out,
with

    stage_us            label (check, union-find, flatten, counts, the roots' compaction), select (mark, the two flag counts and scans, the
                        renumbering), emit (the vertex and triangle writes) at min_triangles = --min-triangles
    extract_emit_us     the emit stage of rgbid_tsdf_extract_emit (rgbid_tsdf_timing) for the same mesh in the same process: the one
                        existing pass that writes these buffers.  Nothing about a ratio is asserted
    components, kept_*  what the labelling found and the selection left

    python tools/mesh_bench.py [--side 256] [--reps 10] [--out profiles/mesh_bench.jsonl]
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


def measure(ctx, name, vol, min_triangles, warmup, reps, extra):
    """extract the volume's mesh `warmup + reps` times with its own timing, then label / select / emit it as often -> one line"""
    from rgbid import mesh as MS
    from rgbid import tsdf as TS
    vol.timing(True)
    emit = []
    for k in range(warmup + reps):
        verts, cols, tris, nrm = vol.extract(1, normals=True)
        ms = vol.timing(True)
        if k >= warmup:
            emit.append(ms["emit"] * 1e-3)
    vol.timing(False)
    cc = MS.Components(ctx, max(verts.shape[0], 1), max(tris.shape[0], 1))
    cc.timing(True)
    ts = {st: [] for st in MS.STAGES}
    for k in range(warmup + reps):
        lab = cc.label(tris, verts.shape[0], tables=False)
        kept = cc.select(min_triangles)
        out = cc.emit(verts, cols, nrm)
        ms = cc.timing(True)
        if k >= warmup:
            for st, v in ms.items():
                ts[st].append(v * 1e-3)
    cc.close()
    med = {k: float(np.median(v)) for k, v in ts.items()}
    line = dict(mesh=name, vertices=int(verts.shape[0]), triangles=int(tris.shape[0]), components=lab["components"], min_triangles=min_triangles,
                kept_components=kept["components"], kept_vertices=kept["vertices"], kept_triangles=kept["triangles"],
                stage_us={k: med[k] * 1e6 for k in MS.STAGES}, total_us=sum(med.values()) * 1e6, extract_emit_us=float(np.median(emit)) * 1e6,
                reps=reps, library=os.path.relpath(TS._lib.LIB_PATH, ROOT), device=torch.cuda.get_device_name(0))
    line.update(extra)
    print(json.dumps(line), flush=True)
    del verts, cols, tris, nrm, out
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--min-triangles", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from cloud_bench import synth_blocks
    from voxel_bench import random_rotation
    from rgbid import cloud as CL
    from rgbid import device, sequence, synth
    from rgbid import tsdf as TS
    rows, cols, side, n = args.rows, args.cols, args.side, args.blocks
    K = (525.0 * cols / 640, 525.0 * rows / 480, cols / 2 - 0.5, rows / 2 - 0.5)
    N = rows * cols
    lines = []
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = device.Context(0)
        # 1. the batch of tools/tsdf_bench.py: shards
        buf = synth_blocks(n, rows, cols, 1000 + n)
        rng = np.random.default_rng(n)
        R = np.stack([random_rotation(rng, 0.3) for _ in range(n)])
        t = rng.uniform(-0.2, 0.2, (n, 3))
        cl = CL.Cloud(ctx, rows, cols, n)
        pts, _ = cl.build([CL.source(buf[k].data_ptr(), R[k], t[k]) for k in range(n)], K, "novel")
        cl.close()
        planes = [buf[k, 4 * N:8 * N].view(torch.float32).view(rows, cols) for k in range(n)]
        colours = [buf[k, N:4 * N].view(rows, cols, 3) for k in range(n)]
        box = np.array(TS.cloud_bounds(pts))
        voxel = float((box[3:] - box[:3]).max() / (side - 1))
        vol = TS.Volume(ctx, side ** 3, n)
        vol.configure(side, side, side, [float(v) for v in box[:3]], voxel, 4.0 * voxel)
        vol.integrate(planes, colours, R, t, K, rows, cols)
        lines.append(measure(ctx, f"batch of {n} blocks", vol, args.min_triangles, args.warmup, args.reps, dict(side=side, voxel_m=voxel)))
        del pts, buf, planes, colours
        # 2. a sphere state in the same volume: one closed component
        vol.configure(side, side, side, [0.0, 0.0, 0.0], 0.05, 0.2)
        ax = torch.arange(side, dtype=torch.float32, device="cuda") * 0.05
        c, r = 0.05 * (side - 1) / 2, 0.05 * side * 0.4
        dist = torch.sqrt((ax[None, None, :] - c) ** 2 + (ax[None, :, None] - c) ** 2 + (ax[:, None, None] - c) ** 2)
        vol.set_state(torch.clamp(dist - r, max=0.2).contiguous(), torch.ones((side,) * 3, dtype=torch.int32, device="cuda"))
        del dist
        lines.append(measure(ctx, "sphere", vol, args.min_triangles, args.warmup, args.reps, dict(side=side, voxel_m=0.05)))
        vol.close()
        torch.cuda.empty_cache()
        # 3. the tracked run of the tests
        Ks = (synth.TUM_K[0] / 4, synth.TUM_K[1] / 4, (synth.TUM_K[2] + 0.5) / 4 - 0.5, (synth.TUM_K[3] + 0.5) / 4 - 0.5)
        seq = synth.make_sequence(24, K=Ks, rows=120, cols=160, device="cuda", noise=False, dropout=0.0, trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
        depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
        _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, Ks, cloud="novel", visratio_odo=0.985, visratio_integr=0.97, keyframe_depth=True,
                                             keyframe_colour=True)
        fused = TS.fuse(ctx, pc.keyframes, Ks, 120, 160, voxel=0.04, points=pc.points, keep_volume=True)
        lines.append(measure(ctx, "tracked run", fused[-1], args.min_triangles, args.warmup, args.reps,
                             dict(side=None, voxel_m=0.04, keyframes=len(pc.keyframes))))
        fused[-1].close()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
