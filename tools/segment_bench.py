#!/usr/bin/env python
"""Keyframe segmentation throughput (include/rgbid_segment.h) on the synthetic scene of rgbid.synth: batches of n frames of 640 x 480
rendered along its camera path, depth with the sequence's noise and dropout, normals from the cross product of the back-projected
depth's central differences (NaN where a neighbour is missing), packed as export blocks.  Each stage is timed with the library's HIP
events (rgbid_segment_timing) after warm-up; one JSON line per batch with the median milliseconds per stage (edges, sort, pass 1, pass 2,
labels, histogram + image + masks), the rounds the slowest keyframe needed in each pass, the segments found, and the bytes the edge and
sort stages move set against 8 TB/s:

    edges   per pixel 20 B read (inverse depth, normals, the point) + 16 B point written + 4 slots x (key + 4 B index) written
    sort    per pass and slot: the keys read twice (histogram, scatter), the indices read once, both written once

    python tools/segment_bench.py [--sizes 1 16 256] [--reps 3] [--out profiles/segment_bench.jsonl]
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

PEAK = 8e12   # B/s


def blocks_from_depth(depth_mm, K):
    """depth [n, rows, cols] in millimetres (0: no measurement) on the device -> packed export blocks uint8 [n, 20 rows cols]"""
    n, rows, cols = depth_mm.shape
    N = rows * cols
    z = depth_mm.to(torch.float32) * 1e-3
    z[z <= 0] = float("nan")
    fx, fy, cx, cy = K
    u = torch.arange(cols, device=z.device, dtype=torch.float32)[None, None, :]
    v = torch.arange(rows, device=z.device, dtype=torch.float32)[None, :, None]
    P = torch.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)
    dx = torch.full_like(P, float("nan")); dy = torch.full_like(P, float("nan"))
    dx[:, :, 1:-1] = P[:, :, 2:] - P[:, :, :-2]
    dy[:, 1:-1] = P[:, 2:] - P[:, :-2]
    nrm = torch.cross(dy, dx, dim=-1)
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    buf = torch.zeros((n, 20 * N), dtype=torch.uint8, device=z.device)
    buf[:, 4 * N:8 * N] = (1.0 / z).reshape(n, N).contiguous().view(torch.uint8)
    buf[:, 8 * N:] = nrm.permute(0, 3, 1, 2).reshape(n, 3 * N).contiguous().view(torch.uint8)
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--window", type=int, default=None, help="the window of the rounds (test hook; default 256)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from rgbid import device, synth
    from rgbid import segment as SG
    rows, cols = args.rows, args.cols
    N = rows * cols
    K = (525.0 * cols / 640, 525.0 * rows / 480, cols / 2 - 0.5, rows / 2 - 0.5)
    lines = []
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = device.Context(0)
        for n in args.sizes:
            seq = synth.make_long_sequence(n, K=K, rows=rows, cols=cols, device="cuda")
            buf = blocks_from_depth(seq["depth"].reshape(n, rows, cols), K)
            del seq
            blocks = [buf[k] for k in range(n)]
            sg = SG.Segmenter(ctx, rows, cols, n, min(N, 16384))
            try:
                sg.segment(blocks, K)
            except SG.SegmentOverflow as e:           # dropout leaves isolated points: tables of the count this batch needs
                sg.close()
                sg = SG.Segmenter(ctx, rows, cols, n, e.count)
            if args.window:
                sg.set_window(args.window)
            sg.timing(True)
            t = {s: [] for s in SG.STAGES}
            for k in range(args.warmup + args.reps):
                labels, counts, sizes, hist, neg, lev = sg.segment(blocks, K)
                if k >= args.warmup:
                    for s, ms in sg.timing(True).items():
                        t[s].append(ms)
            med = {s: float(np.median(v)) for s, v in t.items()}
            rounds = sg.last_rounds()
            points = int((labels >= 0).sum())
            key_b = 4 if n == 1 else 8
            passes = 4 if n == 1 else (32 + (n - 1).bit_length() + 7) // 8
            edge_bytes = n * N * (20 + 16 + 4 * (key_b + 4))
            sort_bytes = passes * 4 * n * N * (2 * key_b + 4 + key_b + 4)
            total = sum(med.values())
            line = {"keyframes": n, "rows": rows, "cols": cols, "points": points, "segments_mean": float(counts.float().mean()),
                    "segments_max": int(counts.max()), "max_segments": sg.max_segments, "window": args.window or SG.MAX_WINDOW, "stage_ms": med, "total_ms": total,
                    "ms_per_keyframe": total / n, "rounds_pass1": rounds[0], "rounds_pass2": rounds[1],
                    "us_per_round_pass1": med["pass1"] * 1e3 / max(rounds[0], 1), "rounds_share_of_total": (med["pass1"] + med["pass2"]) / total,
                    "edge_bytes": edge_bytes, "edge_fraction_of_8TBs": edge_bytes / (med["edges"] * 1e-3) / PEAK,
                    "sort_bytes": sort_bytes, "sort_passes": passes, "sort_fraction_of_8TBs": sort_bytes / (med["sort"] * 1e-3) / PEAK,
                    "reps": args.reps}
            print(json.dumps(line), flush=True)
            lines.append(line)
            sg.close()
            del buf, blocks, labels, counts, sizes, hist, neg, lev
            torch.cuda.empty_cache()
        ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
