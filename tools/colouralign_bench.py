#!/usr/bin/env python
"""Colour alignment stage times (include/rgbid_colouralign.h) on the mesh tools/recolour_bench.py colours: the tracked synthetic run of the
tests (24 frames at 160 x 120, fused with --voxel metres per voxel), seen from 16 and 64 keyframes of 640 x 480 rendered from the same
scene along the same camera path.  The mesh is rasterised at the keyframes' poses (depth only) and one `ColourAligner.run` of --rounds x
--iterations refines the poses with those planes as `surface` and the mesh's normals, the first view held.  Each stage is timed with the
library's HIP events (rgbid_colouralign_timing): the median of `reps` calls after `warmup`; beside it `accumulate` of rgbid_recolour_add
for the same views in the same process, which walks the same (vertex, view) pairs once.  One JSON line per configuration, printed and
written to --out, with

    target_us, system_us, solve_us     per call, summed over its rounds and iterations (solve with the pose pass after it)
    target_us_per_round                target over rounds: one walk over all (vertex, view) pairs
    system_us_per_iteration            system over rounds x iterations
    accumulate_us                      rgbid_recolour_add of the same views (mean mode)
    target_over_accumulate             the target pass against the pass it restates
    ns_per_vertex_view                 system per iteration over lattice vertices x views
    used_pairs                         the used pairs of the last system, summed over the views: what the system pass did arithmetic for

After them the two forms of the target pass ("walk": all views per vertex; "chunks": chunks of 16 views over blocks with integer atomics)
against each other, one line per (views, stride, form) with target_us of one round, the clearing of the state included: 16 keyframes
(one chunk), 64 keyframes and the same 64 taken eight times (512 views), every vertex, every 16th and every 64th.  The library's own choice ("auto") is timed beside them.

    python tools/colouralign_bench.py [--voxel 0.01] [--reps 10] [--out profiles/colouralign_bench.jsonl]
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


def measure(ctx, verts, tris, normals, kfs, Kc, rounds, iterations, warmup, reps, extra):
    from rgbid import colouralign as CA
    from rgbid import raster as RS
    from rgbid import recolour as RC
    V, n_v = len(kfs), verts.shape[0]
    R, t = np.stack([k["R"] for k in kfs]), np.stack([k["t"] for k in kfs])
    colours = [k["colour"] for k in kfs]
    rs = RS.Rasteriser(ctx, n_v, tris.shape[0], ROWS * COLS * V)
    depth = rs.render(verts, tris, R, t, Kc, ROWS, COLS, None, None, outputs=("depth",))["depth"]
    rs.close()
    ca, rc = CA.ColourAligner(ctx, n_v, V), RC.Recolourer(ctx, n_v)
    ca.timing(True); rc.timing(True)
    ts = dict(target=[], system=[], solve=[], accumulate=[])
    res = None
    for k in range(warmup + reps):
        res = ca.run(verts, R, t, Kc, ROWS, COLS, colours, surface=depth, normals=normals, rounds=rounds, iterations=iterations,
                     surface_tolerance=extra["surface_tolerance_m"])
        ms = ca.timing(True)
        rc.begin(n_v, "mean")
        rc.add(verts, R, t, Kc, ROWS, COLS, colours, depth, None, normals, surface_tolerance=extra["surface_tolerance_m"])
        rc.finish()
        acc = rc.timing(True)["accumulate"]
        if k >= warmup:
            for s in CA.STAGES:
                ts[s].append(ms[s] * 1e3)
            ts["accumulate"].append(acc * 1e3)
    ca.close(); rc.close()
    med = {k: float(np.median(v)) for k, v in ts.items()}
    line = dict(mesh="tracked run", vertices=int(n_v), views=V, rows=ROWS, cols=COLS, rounds=rounds, iterations=iterations, stride=1, planes=["surface"],
                normals=normals is not None, target_us=med["target"], system_us=med["system"], solve_us=med["solve"],
                system_us_range=[min(ts["system"]), max(ts["system"])], target_us_per_round=med["target"] / rounds,
                system_us_per_iteration=med["system"] / (rounds * iterations), solve_us_per_iteration=med["solve"] / (rounds * iterations),
                accumulate_us=med["accumulate"], target_over_accumulate=med["target"] / rounds / med["accumulate"],
                ns_per_vertex_view=med["system"] / (rounds * iterations) * 1e3 / (n_v * V), used_pairs=int(res["used"][:, 1].sum()),
                status={CA.STATUS[s]: int((res["status"] == s).sum()) for s in range(len(CA.STATUS))}, reps=reps,
                library=os.path.relpath(CA._lib.LIB_PATH, ROOT), device=torch.cuda.get_device_name(0))
    line.update(extra)
    print(json.dumps(line), flush=True)
    return line


def measure_target(ctx, verts, tris, normals, kfs, Kc, repeat, stride, warmup, reps, extra):
    """the target pass alone in each of its forms -> one line per form"""
    from rgbid import colouralign as CA
    from rgbid import raster as RS
    n_v = verts.shape[0]
    R, t = np.stack([k["R"] for k in kfs]), np.stack([k["t"] for k in kfs])
    rs = RS.Rasteriser(ctx, n_v, tris.shape[0], ROWS * COLS * len(kfs))
    depth = rs.render(verts, tris, R, t, Kc, ROWS, COLS, None, None, outputs=("depth",))["depth"]
    rs.close()
    R, t = np.concatenate([R] * repeat), np.concatenate([t] * repeat)
    colours, surface = [k["colour"] for k in kfs] * repeat, list(depth) * repeat
    V = len(R)
    ca = CA.ColourAligner(ctx, n_v, V)
    ca.timing(True)
    lines = []
    for form in CA.TARGET_FORMS:
        ca.target_form(form)
        ts = []
        for k in range(warmup + reps):
            ca.run(verts, R, t, Kc, ROWS, COLS, colours, surface=surface, normals=normals, rounds=1, iterations=1, stride=stride,
                   surface_tolerance=extra["surface_tolerance_m"])
            ms = ca.timing(True)
            if k >= warmup:
                ts.append(ms["target"] * 1e3)
        n_l = (n_v + stride - 1) // stride
        line = dict(pass_="target", form=form, vertices=int(n_v), stride=stride, lattice=int(n_l), blocks_of_256=(n_l + 255) // 256, views=V, rows=ROWS, cols=COLS,
                    target_us=float(np.median(ts)), target_us_range=[min(ts), max(ts)], ns_per_vertex_view=float(np.median(ts)) * 1e3 / (n_l * V), reps=reps,
                    device=torch.cuda.get_device_name(0))
        line.update(extra)
        print(json.dumps(line), flush=True)
        lines.append(line)
    ca.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--views", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colouralign_bench.jsonl"))
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
            kfs = [dict(R=full["R_wc"][k].cpu().numpy(), t=full["t_wc"][k].cpu().numpy(), colour=full["rgb"][k].contiguous()) for k in range(V)]
            extra = dict(voxel_m=voxel, surface_tolerance_m=2 * voxel)
            lines.append(measure(ctx, verts, tris, normals, kfs, tuple(synth.TUM_K), args.rounds, args.iterations, args.warmup, args.reps, extra))
            sweep = ((1, 1), (8, 1), (1, 16), (8, 16), (1, 64), (8, 64)) if V == max(args.views) else ((1, 1), (1, 64))
            for repeat, stride in sweep:
                lines += measure_target(ctx, verts, tris, normals, kfs, tuple(synth.TUM_K), repeat, stride, args.warmup, args.reps, extra)
            del full, kfs
            torch.cuda.empty_cache()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
