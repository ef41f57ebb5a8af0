#!/usr/bin/env python
"""Feature-preserving denoising throughput (include/rgbid_denoise.h) on the four meshes of tools/smooth_bench.py: section 22's sphere state
in 256^3, the same sphere after vertex clustering with a 2-voxel cell, the tracked synthetic run of the tests and section 22's fan of 4 096
triangles, every face of which merges the hub's row of 4 096: the serial worst case.  Each stage is timed with the library's HIP events
(rgbid_denoise_timing): the median of `reps` plan + normals + vertices calls after `warmup`; Taubin's pass (rgbid_smooth_timing) is timed
on the same mesh in the same process for comparison; one JSON line per mesh, printed and written to --out, with

    plan_us             check, corner keys, the sort, face table, offsets, the counts; the host's wait for the first count is not in it;
                        plan_wall_us is the host clock around the whole synchronising plan call
    normal_pass_us      (normals_us - raw_us) / normal iterations, where raw_us is a normals call with no iteration: the raw normals alone
    vertex_pass_us      vertices_us / vertex iterations; all passes are enqueued without a host wait
    normal_pass_bytes   what one normal pass must move once: 48 n_t + 4 (n_v + 1) (normals read and written, triangles, face table, offsets)
    vertex_pass_bytes   what one vertex pass must move once: 28 n_v + 36 n_t + 4 (positions read and written, offsets, face table,
                        triangles, normals); *_share_of_8TBps: those bytes over the pass's time against 8 TB/s
    smooth_pass_us      one pass of Taubin's filter over the same mesh

    python tools/denoise_bench.py [--side 256] [--normal-iterations 5] [--vertex-iterations 10] [--reps 10] [--out profiles/denoise_bench.jsonl]
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


def smooth_pass_us(ctx, verts, tris, warmup, reps):
    """the median time of one pass of Taubin's filter on the mesh"""
    from rgbid import smooth as SO
    sm = SO.Smoother(ctx, max(verts.shape[0], 1), max(tris.shape[0], 1))
    sm.timing(True)
    sm.plan(tris, verts.shape[0])
    ts = []
    for k in range(warmup + reps):
        sm.run(verts, 10)
        ms = sm.timing(True)
        if k >= warmup:
            ts.append(ms["run"] * 1e3 / 20)
    sm.close()
    return float(np.median(ts))


def measure(ctx, name, verts, tris, normal_iterations, vertex_iterations, threshold, warmup, reps, extra):
    """plan + normals + vertices `warmup + reps` times on the mesh -> one line"""
    from rgbid import denoise as DN
    dn = DN.Denoiser(ctx, max(verts.shape[0], 1), max(tris.shape[0], 1))
    dn.timing(True)
    ts, wall, raw = {st: [] for st in DN.STAGES}, [], []
    for k in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        plan = dn.plan(tris, verts.shape[0])
        t1 = time.perf_counter()
        dn.normals(verts, 0, threshold)
        raw_ms = dn.timing(True)["normals"]
        nrm = dn.normals(verts, normal_iterations, threshold)
        dn.vertices(verts, nrm, vertex_iterations)
        ms = dn.timing(True)
        if k >= warmup:
            wall.append(t1 - t0)
            raw.append(raw_ms * 1e-3)
            for st, v in ms.items():
                ts[st].append(v * 1e-3)
    dn.close()
    med = {k: float(np.median(v)) for k, v in ts.items()}
    raw_us = float(np.median(raw)) * 1e6
    n_v, n_t = int(verts.shape[0]), int(tris.shape[0])
    normal_pass_us = (med["normals"] * 1e6 - raw_us) / max(normal_iterations, 1)
    vertex_pass_us = med["vertices"] * 1e6 / max(vertex_iterations, 1)
    normal_bytes, vertex_bytes = 48 * n_t + 4 * (n_v + 1), 28 * n_v + 36 * n_t + 4
    line = dict(mesh=name, vertices=n_v, triangles=n_t, normal_iterations=normal_iterations, vertex_iterations=vertex_iterations, threshold=threshold,
                counts=plan, plan_us=med["plan"] * 1e6, plan_wall_us=float(np.median(wall)) * 1e6, raw_us=raw_us, normals_us=med["normals"] * 1e6,
                vertices_us=med["vertices"] * 1e6, normal_pass_us=normal_pass_us, vertex_pass_us=vertex_pass_us, normal_pass_bytes=normal_bytes,
                vertex_pass_bytes=vertex_bytes, normal_pass_share_of_8TBps=normal_bytes / (normal_pass_us * 1e-6) / 8e12,
                vertex_pass_share_of_8TBps=vertex_bytes / (vertex_pass_us * 1e-6) / 8e12, smooth_pass_us=smooth_pass_us(ctx, verts, tris, warmup, reps),
                reps=reps, library=os.path.relpath(DN._lib.LIB_PATH, ROOT), device=torch.cuda.get_device_name(0))
    line.update(extra)
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--normal-iterations", type=int, default=5)
    ap.add_argument("--vertex-iterations", type=int, default=10)
    ap.add_argument("--threshold", type=float, default=0.4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from rgbid import device, sequence, synth
    from rgbid import tsdf as TS
    side, lines = args.side, []
    run = lambda name, v, t, extra: lines.append(measure(ctx, name, v, t, args.normal_iterations, args.vertex_iterations, args.threshold, args.warmup,
                                                         args.reps, extra))
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
        # 3. the fan: 4 096 triangles around one hub; every face merges the hub's row of 4 096, one thread walks it in the vertex pass
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
