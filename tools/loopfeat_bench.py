#!/usr/bin/env python
"""Loop-feature stage timing (include/rgbid_loopfeat.h) with the library's HIP events (rgbid_loopfeat_timing), median over --reps after
warm-up; one JSON line per case with the microseconds per stage and a byte / operation model beside it:

    features, n keyframes of rows x cols, k keypoints each (1 000 at most)
      response  rows cols (1 read of the grey byte through a 24 x 24 tile, x 2.25 halo) + 4 rows cols written; 49 x 3 integer MACs per pixel
      select    9 x 4 rows cols read (the 8 neighbours come from cache), 4 rows cols inverse depth; rank by counting: c^2 compares per cell
      describe  per keypoint 1 089 patch bytes, 709 moment MACs, 512 box sums of 25 bytes from LDS, 120 bytes written
    match, P pairs of a query and a candidate with k keypoints: 32 k bytes staged per pair + 32 k read per pair; k^2 x 4 (XOR, popcount,
      add) on 64-bit words = 12 k^2 integer operations per pair; peak taken as 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3 T 32-bit ops/s
      (a 64-bit popcount is two)
    ransac, P pairs of m matches, I iterations: I m votes of 2 errors, about 230 FP64 operations per error; 144 m bytes staged per pass of
      256 hypotheses; peak taken as 78.6 TFLOP/s FP64 vector

    with --levels N --scale S (a feature pyramid): the pyramid as a stage of its own (1.7 B per destination pixel: 4 taps of which about
      1.44 source bytes are new, 1 written, levels 1 .. L - 1 hold about 2.1 x the pixels of level 0 at 1.2), the other feature stages over
      all levels' pixels, features per keyframe, and the match stage at the keypoint counts the levels really yield

    python tools/loopfeat_bench.py [--keyframes 64 256] [--pairs 64 1024] [--reps 5] [--levels 8 --scale 1.2]
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

INT_OPS = 256 * 4 * 16 * 2.4e9
FP64_FLOPS = 78.6e12
PEAK_BPS = 8.0e12


def textured(r, rows, cols):
    img = r.integers(90, 110, (rows, cols)).astype(np.int32)
    for _ in range(rows * cols // 300):
        y, x = int(r.integers(0, rows - 4)), int(r.integers(0, cols - 4))
        img[y:y + int(r.integers(3, 24)), x:x + int(r.integers(3, 24))] = int(r.integers(0, 256))
    return img.clip(0, 255).astype(np.uint8)


def median_ms(lf, fn, stages, reps, warmup):
    """-> ({stage: median ms}, {stage: (min, max) ms}); the stage "pyramid" comes from the library's own call"""
    out = {s: [] for s in stages}
    for k in range(warmup + reps):
        fn()
        ms = lf.timing(True)
        if "pyramid" in out:
            ms["pyramid"] = lf.timing_pyramid()
        if k >= warmup:
            for s in stages:
                out[s].append(ms[s])
    return {s: float(np.median(v)) for s, v in out.items()}, {s: (float(min(v)), float(max(v))) for s, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--pairs", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--max-keypoints", type=int, default=1000)
    ap.add_argument("--levels", type=int, default=1, help="pyramid levels of the feature extractor (1 .. 8)")
    ap.add_argument("--scale", type=float, default=1.2, help="scale between neighbouring levels")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    from rgbid import device
    from rgbid import loopfeat as LF
    rows, cols, mk = args.rows, args.cols, args.max_keypoints
    K = (525.0 * cols / 640, 525.0 * rows / 480, cols / 2 - 0.5, rows / 2 - 0.5)
    r = np.random.default_rng(0)
    ctx = device.Context(0)
    lf = LF.LoopFeat(ctx, rows, cols, mk, args.levels, args.scale)
    px_all = sum(l[0] * l[1] for l in lf.levels)           # pixels of all levels
    stages = (("pyramid",) if len(lf.levels) > 1 else ()) + ("response", "select", "describe")
    lf.timing(True)
    base = [textured(r, rows, cols) for _ in range(8)]
    for n in args.keyframes:
        grey = torch.from_numpy(np.stack([base[k % 8] for k in range(n)])).cuda()
        grey = torch.roll(grey, shifts=3, dims=2) if n % 2 else grey
        w = torch.full((n, rows, cols), 0.8, dtype=torch.float32, device="cuda")
        holder = {}
        ms, spread = median_ms(lf, lambda: holder.__setitem__("f", lf.extract(grey, w, K)), stages, args.reps, args.warmup)
        feats = holder["f"]
        kp = float(feats.counts.float().mean())
        px = px_all
        model = dict(pyramid_bytes=n * (px_all - rows * cols) * 1.7, response_bytes=n * px * (2.25 + 4), select_bytes=n * px * 8,
                     describe_bytes=n * kp * (1089 + 120))
        print(json.dumps(dict(case="features", keyframes=n, rows=rows, cols=cols, levels=len(lf.levels), scale=args.scale,
                              pixels_over_level0=px_all / (rows * cols), keypoints_mean=kp,
                              us={k: 1e3 * v for k, v in ms.items()}, us_min_max={k: [1e3 * a, 1e3 * b] for k, (a, b) in spread.items()},
                              us_per_keyframe=1e3 * sum(ms.values()) / n,
                              us_per_keyframe_by_stage={k: 1e3 * v / n for k, v in ms.items()},
                              frac_of_8TBps={s: model[s + "_bytes"] / (ms[s] * 1e-3) / PEAK_BPS for s in ms})))
        pairs = LF.all_pairs(n, 3)
        ms, _ = median_ms(lf, lambda: lf.match(feats, pairs, lists=False), ("match",), args.reps, args.warmup)
        ops = len(pairs) * 12.0 * kp * kp
        print(json.dumps(dict(case="match_all_pairs", keyframes=n, pairs=len(pairs), keypoints_mean=kp, us=1e3 * ms["match"],
                              int_ops=ops, frac_of_int_peak=ops / (ms["match"] * 1e-3) / INT_OPS, bytes=len(pairs) * 64.0 * kp)))
    n = max(args.keyframes)
    iters = LF.num_iters()
    for P in args.pairs:
        pairs = [(int(q), int(c)) for q, c in zip(r.integers(1, n, P), r.integers(0, n, P))]
        m, mc = lf.match(feats, pairs)
        ms, _ = median_ms(lf, lambda: lf.ransac(feats, pairs, m, mc), ("ransac",), args.reps, args.warmup)
        mm = float(mc.float().mean())
        flops = P * iters * mm * 2 * 230.0
        print(json.dumps(dict(case="ransac", pairs=P, iterations=iters, matches_mean=mm, us=1e3 * ms["ransac"], fp64_flops=flops,
                              frac_of_fp64_peak=flops / (ms["ransac"] * 1e-3) / FP64_FLOPS, staged_bytes=P * 144.0 * mm)))
    lf.close()
    ctx.close()


if __name__ == "__main__":
    main()
