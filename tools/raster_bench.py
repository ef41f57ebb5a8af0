#!/usr/bin/env python
"""Mesh rasteriser throughput (include/rgbid_raster.h) at 640 x 480 with 1 and 16 views on four meshes: section 22's sphere state in
256^3 (591 062 vertices, 1 182 120 triangles), the same sphere after vertex clustering with a 2-voxel cell, the tracked synthetic run of
the tests (24 frames at 160 x 120, a 0.04 m voxel; its keyframes' poses, repeated to 16) and one triangle that fills the image.  Each
stage is timed with the library's HIP events (rgbid_raster_timing): the median of `reps` calls after `warmup`; one JSON line per mesh
and view count, printed and written to --out, with

    project_us, setup_us, large_us, resolve_us   the four stages (the clear is in project, the list's compaction in large)
    fragments_per_s                              covered pixel tests over setup + large
    large_share                                  drawn (triangle, view) pairs whose box holds more than SMALL_BOX pixels, over the drawn
                                                 ones (from the projected mesh on the host; the library does not count them)
    raycast_us                                   Volume.raycast of the same surface at the same views in the same process (depth only, step
                                                 = voxel), where there is a volume: the one other way to a depth image of this surface

    python tools/raster_bench.py [--side 256] [--reps 10] [--out profiles/raster_bench.jsonl]
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
K = (525.0, 525.0, 319.5, 239.5)


def large_share(RS, verts, tris, R, t, Kc, rows, cols, z_min, z_max):
    """the share of the drawn (triangle, view) pairs that take the large path, with torch on the device in float64 / int64: a figure about
    the workload, not a restatement of the contract (a vertex on a rounding boundary may fall the other way)"""
    v = verts.double()
    tr = tris.long() & 0xFFFFFFFF
    drawn = large = 0
    for Rw, tw in zip(R, t):
        Rw, tw = torch.tensor(Rw, dtype=torch.float64, device=v.device), torch.tensor(tw, dtype=torch.float64, device=v.device)
        cam = (v - tw) @ Rw
        Z = cam[:, 2]
        ok = torch.isfinite(cam).all(1) & (Z >= z_min) & (Z <= z_max)
        xs = torch.floor((Kc[0] * cam[:, 0] / Z + Kc[2]) * RS.SUB + 0.5)
        ys = torch.floor((Kc[1] * cam[:, 1] / Z + Kc[3]) * RS.SUB + 0.5)
        ok &= (xs.abs() <= 2 ** 23) & (ys.abs() <= 2 ** 23)
        xs, ys = torch.where(ok, xs, 0.0).long(), torch.where(ok, ys, 0.0).long()
        a, b, c = tr[:, 0], tr[:, 1], tr[:, 2]
        A = (xs[b] - xs[a]) * (ys[c] - ys[a]) - (ys[b] - ys[a]) * (xs[c] - xs[a])
        tx, ty = torch.stack([xs[a], xs[b], xs[c]]), torch.stack([ys[a], ys[b], ys[c]])
        x0 = torch.clamp(-((-tx.min(0).values) // RS.SUB), min=0); x1 = torch.clamp(tx.max(0).values // RS.SUB, max=cols - 1)
        y0 = torch.clamp(-((-ty.min(0).values) // RS.SUB), min=0); y1 = torch.clamp(ty.max(0).values // RS.SUB, max=rows - 1)
        is_drawn = ok[a] & ok[b] & ok[c] & (A != 0) & (x0 <= x1) & (y0 <= y1)
        drawn += int(is_drawn.sum())
        large += int((is_drawn & ((x1 - x0 + 1) * (y1 - y0 + 1) > RS.SMALL_BOX)).sum())
    return large / drawn if drawn else 0.0


def measure(ctx, name, verts, tris, R, t, Kc, rows, cols, warmup, reps, extra, volume=None, z_min=0.05, z_max=20.0):
    from rgbid import raster as RS
    V = len(R)
    rs = RS.Rasteriser(ctx, max(verts.shape[0], 1), max(tris.shape[0], 1), rows * cols * V)
    rs.timing(True)
    ts = {st: [] for st in RS.STAGES}
    for k in range(warmup + reps):
        rs.render(verts, tris, R, t, Kc, rows, cols, None, None, z_min, z_max, outputs=("depth",))
        ms = rs.timing(True)
        if k >= warmup:
            for st, v in ms.items():
                ts[st].append(v * 1e3)
    counts = rs.counts()
    rs.close()
    med = {k: float(np.median(v)) for k, v in ts.items()}
    total = {k: sum(c[k] for c in counts) for k in RS.COUNTS}
    line = dict(mesh=name, vertices=int(verts.shape[0]), triangles=int(tris.shape[0]), views=V, rows=rows, cols=cols, counts=total,
                project_us=med["project"], setup_us=med["setup"], large_us=med["large"], resolve_us=med["resolve"],
                fragments_per_s=total["fragments"] / ((med["setup"] + med["large"]) * 1e-6),
                large_share=large_share(RS, verts, tris, R, t, Kc, rows, cols, z_min, z_max), reps=reps,
                library=os.path.relpath(RS._lib.LIB_PATH, ROOT), device=torch.cuda.get_device_name(0))
    if volume is not None:
        volume.raycast_timing(True)
        us = []
        for k in range(warmup + reps):
            volume.raycast(R, t, Kc, rows, cols, None, 1, z_min, z_max, outputs=("depth",))
            ms = volume.raycast_timing(True)
            if k >= warmup:
                us.append(list(ms.values())[0] * 1e3 if isinstance(ms, dict) else float(ms) * 1e3)
        line["raycast_us"] = float(np.median(us))
        line["raycast_over_raster"] = line["raycast_us"] / sum(med.values())
    line.update(extra)
    print(json.dumps(line), flush=True)
    return line


def orbit(centre, radius, n):
    """n world poses on a circle around `centre` in the plane y = centre.y, each looking at it (camera z towards the centre, y down)"""
    R, t = [], []
    for k in range(n):
        a = 2 * np.pi * k / max(n, 1) * 0.25                  # a quarter turn: neighbouring views overlap as keyframes do
        pos = np.array(centre) + radius * np.array([np.sin(a), 0.0, -np.cos(a)])
        z = (np.array(centre) - pos) / radius
        x = np.cross([0.0, 1.0, 0.0], z); x /= np.linalg.norm(x)
        R.append(np.stack([x, np.cross(z, x), z], 1)); t.append(pos)
    return np.stack(R), np.stack(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from rgbid import device, sequence, synth
    from rgbid import tsdf as TS
    side, lines = args.side, []
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = device.Context(0)
        # 1. section 22's sphere and what vertex clustering at 2 voxels leaves of it, beside the ray cast of the same volume
        vol = TS.Volume(ctx, side ** 3, 16)
        vol.configure(side, side, side, [0.0, 0.0, 0.0], 0.05, 0.2)
        ax = torch.arange(side, dtype=torch.float32, device="cuda") * 0.05
        c, r = 0.05 * (side - 1) / 2, 0.05 * side * 0.4
        dist = torch.sqrt((ax[None, None, :] - c) ** 2 + (ax[None, :, None] - c) ** 2 + (ax[:, None, None] - c) ** 2)
        vol.set_state(torch.clamp(dist - r, max=0.2).contiguous(), torch.ones((side,) * 3, dtype=torch.int32, device="cuda"))
        del dist
        verts, _, tris = vol.extract(1, colours=False)
        sv, _, st = vol.extract(1, colours=False, simplify=0.1)
        for V in (1, 16):
            R, t = orbit((c, c, c), 2.2 * r, V)
            extra = dict(side=side, voxel_m=0.05)
            lines.append(measure(ctx, "sphere", verts, tris, R, t, K, ROWS, COLS, args.warmup, args.reps, extra, vol))
            lines.append(measure(ctx, "sphere simplified at 2 voxels", sv, st, R, t, K, ROWS, COLS, args.warmup, args.reps, extra, vol))
        vol.close()
        del verts, tris, sv, st
        torch.cuda.empty_cache()
        # 2. the tracked run of the tests, seen through a 640 x 480 camera of the same field of view from its keyframes' poses
        Ks = (synth.TUM_K[0] / 4, synth.TUM_K[1] / 4, (synth.TUM_K[2] + 0.5) / 4 - 0.5, (synth.TUM_K[3] + 0.5) / 4 - 0.5)
        seq = synth.make_sequence(24, K=Ks, rows=120, cols=160, device="cuda", noise=False, dropout=0.0, trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
        depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
        _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, Ks, cloud="novel", visratio_odo=0.985, visratio_integr=0.97, keyframe_depth=True,
                                             keyframe_colour=True)
        fused = TS.fuse(ctx, pc.keyframes, Ks, 120, 160, voxel=0.04, points=pc.points, keep_volume=True)
        verts, tris, volume = fused[0], fused[2], fused[-1]
        for V in (1, 16):
            kfs = [pc.keyframes[k % len(pc.keyframes)] for k in range(V)]
            R, t = np.stack([np.asarray(k["R"]) for k in kfs]), np.stack([np.asarray(k["t"]) for k in kfs])
            lines.append(measure(ctx, "tracked run", verts, tris, R, t, tuple(synth.TUM_K), ROWS, COLS, args.warmup, args.reps,
                                 dict(side=None, voxel_m=0.04, keyframes=len(pc.keyframes)), volume if V <= volume.max_views else None))
        volume.close()
        # 3. one triangle that fills the image
        tri = torch.tensor([[0, 1, 2]], dtype=torch.int32, device="cuda")
        big = torch.tensor([[-20.0, -20.0, 2.0], [40.0, -20.0, 3.0], [-20.0, 40.0, 4.0]], device="cuda")
        for V in (1, 16):
            lines.append(measure(ctx, "one triangle", big, tri, np.stack([np.eye(3)] * V), np.zeros((V, 3)), K, ROWS, COLS, args.warmup, args.reps,
                                 dict(side=None, voxel_m=None)))
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
