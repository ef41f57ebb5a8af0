#!/usr/bin/env python
"""Keyframe point-cloud throughput (include/rgbid_cloud.h): plan (count + scans + offsets to the host) and emit timed separately with
HIP events on the context's stream, after warm-up, over batches of n synthesised 640 x 480 export blocks (~70 % valid pixels, overlap mask
0 on half of them).  Prints one JSON line: per batch size the microseconds per keyframe of each pass and the fraction of 8 TB/s the
pass's algorithmic bytes reach -- plan: iD + normal x (+ mask in the novel mode) = 8 (9) B/px read; emit: 20 B/px read + 32 B per point
written.

    python tools/cloud_bench.py [--sizes 16 256] [--mode novel|all] [--reps 30] [--rows 480 --cols 640]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rgbid-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

PEAK_BPS = 8.0e12


def synth_blocks(n, rows, cols, seed):
    """n distinct packed blocks on the device: iD ~U(0.2, 2.2) with 30 % NaN, normals ~N(0, 1), random colours, mask 0 on ~half"""
    N = rows * cols
    g = torch.Generator(device="cuda").manual_seed(seed)
    buf = torch.empty((n, 20 * N), dtype=torch.uint8, device="cuda")
    for k in range(n):
        iD = torch.rand(N, generator=g, device="cuda") * 2.0 + 0.2
        iD[torch.rand(N, generator=g, device="cuda") < 0.3] = float("nan")
        buf[k, :N] = (torch.rand(N, generator=g, device="cuda") < 0.5).to(torch.uint8)
        buf[k, N:4 * N] = torch.randint(0, 256, (3 * N,), generator=g, device="cuda", dtype=torch.uint8)
        buf[k, 4 * N:8 * N] = iD.view(torch.uint8)
        buf[k, 8 * N:] = torch.randn(3 * N, generator=g, device="cuda").view(torch.uint8)
    torch.cuda.synchronize()
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--mode", choices=["novel", "all"], default="novel")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--cols", type=int, default=640)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from rgbid import cloud as CL
    from rgbid import device
    rows, cols = args.rows, args.cols
    N = rows * cols
    K = (525.0 * cols / 640, 525.0 * rows / 480, cols / 2 - 0.5, rows / 2 - 0.5)
    stream = torch.cuda.Stream()
    out = {"rows": rows, "cols": cols, "mode": args.mode, "reps": args.reps, "peak_TBps": PEAK_BPS / 1e12}
    with torch.cuda.stream(stream):
        ctx = device.Context(0)              # shares `stream`: the events below time exactly the context's work
        for n in args.sizes:
            buf = synth_blocks(n, rows, cols, 1000 + n)
            rng = np.random.default_rng(n)
            srcs = []
            for k in range(n):
                q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
                srcs.append(CL.source(buf[k].data_ptr(), q, rng.normal(size=3)))
            cl = CL.Cloud(ctx, rows, cols, n)
            offsets = cl.plan(srcs, K, args.mode)
            M = int(offsets[-1])
            pts = torch.empty((M, 32), dtype=torch.uint8, device="cuda")
            for _ in range(args.warmup):
                cl.plan(srcs, K, args.mode)
                cl.emit(pts)
            ctx.sync()
            t_plan, t_emit = [], []
            for _ in range(args.reps):
                e0, e1, e2 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                cl.plan(srcs, K, args.mode)            # synchronises
                e1.record(stream)
                cl.emit(pts)
                e2.record(stream)
                e2.synchronize()
                t_plan.append(e0.elapsed_time(e1) * 1e-3); t_emit.append(e1.elapsed_time(e2) * 1e-3)
            cl.close()
            tp, te = float(np.median(t_plan)), float(np.median(t_emit))
            plan_bytes = (9 if args.mode == "novel" else 8) * N * n
            emit_bytes = 20 * N * n + 32 * M
            out[f"n{n}"] = {
                "points": M, "valid_fraction": M / (n * N),
                "plan_us_per_kf": tp / n * 1e6, "emit_us_per_kf": te / n * 1e6,
                "plan_us_spread": [float(np.min(t_plan)) * 1e6, float(np.max(t_plan)) * 1e6],
                "emit_us_spread": [float(np.min(t_emit)) * 1e6, float(np.max(t_emit)) * 1e6],
                "plan_frac_8TBps": plan_bytes / tp / PEAK_BPS, "emit_frac_8TBps": emit_bytes / te / PEAK_BPS,
                "emit_fp64_flop": 60 * M,
            }
            del buf, pts
            torch.cuda.empty_cache()
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
