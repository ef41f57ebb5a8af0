#!/usr/bin/env python
"""Vocabulary stage timing (include/rgbid_bow.h) with the library's HIP events (rgbid_bow_timing), median over --reps after warm-up, beside
the all-pairs matching it replaces (rgbid_loopfeat_timing), and the two proposals end to end (wall clock around loopfeat.propose, which
synchronises), alternated --rounds times in one session on one device.  One JSON line per case; --out appends the lines to a file.

    keyframes  features are extracted from 64 textured images and repeated to the keyframe count (the stages' work depends on the counts
               of keypoints and words, not on which keyframes look alike)
    all-pairs  above --all-pairs-full keyframes the all-pairs matching is run once, without warm-up, and the line says so (reps = 1); when
               its pair list or its counts cannot be allocated the line says that instead

    python tools/bow_bench.py [--keyframes 256 1024 4096] [--reps 5] [--rounds 2] [--out profiles/bow_bench.jsonl]

--quality N: instead of timing, N keyframes taken every --stride frames from the bounded synthetic path at 160 x 120 (it revisits itself):
the pairs the all-pairs proposal selects, the share of them inside the shortlist for T = 4, 8, 16, and the loops that pass RANSAC and its
gates under either proposal."""
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


def emit(out, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def median_ms(obj, fn, stage, reps, warmup):
    v = []
    for k in range(warmup + reps):
        fn()
        ms = obj.timing(True)[stage]
        if k >= warmup:
            v.append(ms)
    return float(np.median(v)), (float(min(v)), float(max(v)))


def wall_ms(fn, reps, warmup):
    v = []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            v.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(v))


def timing(args):
    from loopfeat_bench import textured
    from rgbid import bow as BW
    from rgbid import device
    from rgbid import loopfeat as LF
    rows, cols, mk = 480, 640, args.max_keypoints
    K = (525.0, 525.0, 319.5, 239.5)
    r = np.random.default_rng(0)
    ctx = device.Context(0)
    lf = LF.LoopFeat(ctx, rows, cols, mk)
    base = lf.extract(np.stack([textured(r, rows, cols) for _ in range(64)]), np.full((64, rows, cols), 0.8, np.float32), K)
    lf.timing(True)
    for rnd in range(args.rounds):
        for n in args.keyframes:
            idx = torch.arange(n, device="cuda") % 64
            feats = LF.Features(base.kps[idx].contiguous(), base.counts[idx].contiguous())
            kp = float(feats.counts.float().mean())
            voc = BW.Vocabulary(ctx, args.k, args.depth)
            voc.timing(True)
            t_train, _ = median_ms(voc, lambda: voc.train(feats), "train", 1 if n > 1024 else args.reps, 0 if n > 1024 else 1)
            nodes = len(voc.export()["children"])
            hold = {}
            t_tr, s_tr = median_ms(voc, lambda: hold.__setitem__("b", voc.transform(feats)), "transform", args.reps, 1)
            t_sl, s_sl = median_ms(voc, lambda: voc.shortlist(hold["b"], 3, args.T), "shortlist", args.reps, 1)
            cand, _ = voc.shortlist(hold["b"], 3, args.T)
            sp = BW.shortlist_pairs(cand)
            t_ms, _ = median_ms(lf, lambda: lf.match(feats, sp, lists=False), "match", args.reps, 1)
            t_prop_bow = wall_ms(lambda: LF.propose(lf, feats, shortlist=voc, shortlist_size=args.T), args.reps, 1)
            emit(args.out, case="bow", round=rnd, keyframes=n, keypoints_mean=kp, k=args.k, depth=args.depth, nodes=nodes, T=args.T,
                 words_mean=float(hold["b"].counts.float().mean()), train_ms=t_train, transform_ms=t_tr, transform_min_max=s_tr,
                 shortlist_ms=t_sl, shortlist_min_max=s_sl, shortlist_pairs=len(sp), match_shortlist_ms=t_ms,
                 device_total_ms=t_tr + t_sl + t_ms, propose_wall_ms=t_prop_bow)
            n_all = sum(1 + max(q - 2, 0) for q in range(1, n))
            full = n <= args.all_pairs_full
            try:
                ap = LF.all_pairs(n, 3)
                t_all, _ = median_ms(lf, lambda: lf.match(feats, ap, lists=False), "match", args.reps if full else 1, 1 if full else 0)
                t_prop_all = wall_ms(lambda: LF.propose(lf, feats), args.reps if full else 1, 1 if full else 0)
                emit(args.out, case="all_pairs", round=rnd, keyframes=n, pairs=len(ap), pair_list_bytes=8 * len(ap), reps=args.reps if full else 1,
                     match_ms=t_all, propose_wall_ms=t_prop_all)
            except (MemoryError, RuntimeError) as e:
                emit(args.out, case="all_pairs", round=rnd, keyframes=n, pairs=n_all, pair_list_bytes=8 * n_all, not_run=str(e)[:200])
            voc.close()
    lf.close()
    ctx.close()


def quality(args):
    from rgbid import bow as BW
    from rgbid import device, synth
    from rgbid import loopfeat as LF
    from rgbid.posegraph import grey_from_colors
    rows, cols = 120, 160
    K = (synth.TUM_K[0] / 4, synth.TUM_K[1] / 4, (synth.TUM_K[2] + 0.5) / 4 - 0.5, (synth.TUM_K[3] + 0.5) / 4 - 0.5)
    n = args.quality
    seq = synth.make_long_sequence(n * args.stride, K=K, rows=rows, cols=cols, device="cuda")
    d = seq["depth"][::args.stride][:n].cpu().numpy()      # millimetres
    d = (d.view(np.uint16) if d.dtype == np.int16 else d).astype(np.float32)
    w = np.where(d > 0, 1000.0 / np.maximum(d, 1.0), 0.0).astype(np.float32)
    grey = grey_from_colors(seq["rgb"][::args.stride][:n].cpu().numpy())
    ctx = device.Context(0)
    lf = LF.LoopFeat(ctx, rows, cols, 1000)
    feats = lf.extract(grey, w, K)
    kps, counts = feats.numpy()

    def verified(pairs):
        if not pairs:
            return []
        m, mc = lf.match(feats, pairs)
        res = lf.ransac(feats, pairs, m, mc)
        mh, mch = m.cpu().numpy().view(LF.MATCH_DTYPE).reshape(len(pairs), -1), mc.cpu().numpy()
        return [p for k, p in enumerate(pairs)
                if res["best"][k] >= 0 and LF.gate(kps[p[0]], kps[p[1]], mh[k, :mch[k]], res["mask"][k], rows, cols)[0]]

    pairs_all, _ = LF.propose(lf, feats)
    ok_all = verified(pairs_all)
    voc = BW.Vocabulary(ctx, args.k, args.depth)
    voc.train(feats)
    bow = voc.transform(feats)
    for T in (4, 8, 16):
        cand, _ = voc.shortlist(bow, 3, T)
        sp = set(BW.shortlist_pairs(cand))
        pairs_b, _ = LF.propose(lf, feats, shortlist=voc, shortlist_size=T)
        ok_b = verified(pairs_b)
        emit(args.out, case="quality", keyframes=n, stride=args.stride, keypoints_mean=float(counts.mean()), k=args.k, depth=args.depth,
             nodes=len(voc.export()["children"]), T=T, all_pairs_selected=len(pairs_all), inside_shortlist=sum(p in sp for p in pairs_all),
             shortlist_selected=len(pairs_b), selected_in_common=len(set(pairs_b) & set(pairs_all)), all_pairs_verified=len(ok_all),
             shortlist_verified=len(ok_b), verified_in_common=len(set(ok_b) & set(ok_all)))
    voc.close(); lf.close(); ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--max-keypoints", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--T", type=int, default=8)
    ap.add_argument("--all-pairs-full", type=int, default=1024, help="largest keyframe count at which the all-pairs matching gets warm-up and --reps")
    ap.add_argument("--quality", type=int, default=0, metavar="N")
    ap.add_argument("--stride", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    quality(args) if args.quality else timing(args)


if __name__ == "__main__":
    main()
