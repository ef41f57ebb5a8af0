"""Time the batched pose-graph solver (include/rgbid_posegraph.h): G graphs x T frames x K keyframes x L loops.

Prints one JSON line: the median device time of a full optimisation (HIP events from the first upload to the last read-back), the median
host wall time of the call (which adds the host's structure building), the median device time per kernel kind (HIP events), the FP64 rate of the reduced factorisations against the 78.6 TFLOP/s vector spec and the
bytes of the linearise and segment kernels against 8 TB/s.  16 distinct random graphs are tiled to G (rgbid.posegraph.synthetic_graph).

    python tools/posegraph_bench.py --graphs 2048 --frames 1000 --keyframes 64 --loops 8 [--single] [--reps 5] [--reduced dense|envelope]
    python tools/posegraph_bench.py --graphs 1 --frames 12000 --keyframes 5400 --loops 48 --reduced envelope      # one long graph
    python tools/posegraph_bench.py --graphs 1 --frames 3000 --keyframes 1000 --loops 500 --reduced envelope      # loop-heavy

--reduced chooses the reduced-system solver (rgbid_pg_set_limits): dense = the default (graphs above 256 separators are refused), envelope =
every graph by the envelope factorisation, no cap.  The line then also reports the envelope's block count against the dense ns^2 and the
histogram of its row widths.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rgbid-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from rgbid import device, posegraph as PG  # noqa: E402
from rgbid.posegraph import synthetic_graph  # noqa: E402

FP64_VECTOR_TFLOPS = 78.6
HBM_TBPS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--keyframes", type=int, default=64)
    ap.add_argument("--loops", type=int, default=8)
    ap.add_argument("--single", action="store_true", help="single-level schedule (default: multilevel)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reduced", choices=("dense", "envelope"), default="dense", help="reduced-system solver (envelope: no separator cap)")
    a = ap.parse_args()
    r = np.random.default_rng(0)
    proto = [synthetic_graph(r, a.frames, K=a.keyframes, L=a.loops, drift=0.01, noise=1e-4)[:2] for _ in range(min(16, a.graphs))]
    graphs = [proto[g % len(proto)] for g in range(a.graphs)]
    ranges = np.zeros(len(graphs), PG.GRAPH_DTYPE)
    v = e = 0
    for g, (P, E) in enumerate(graphs):
        ranges[g] = (v, len(P), e, len(E))
        v += len(P)
        e += len(E)
    P = np.concatenate([p for p, _ in graphs])
    E = np.concatenate([x for _, x in graphs])
    ctx = device.Context(0)
    pg = PG.PoseGraph(ctx)
    ml = not a.single
    if a.reduced == "envelope":
        pg.set_limits(max(PG.MAX_SEPARATORS, a.frames), 1)
    # the reduced systems of the first stage with separators: blocks the envelope stores against the dense ns^2, and the row widths
    blocks = dense_blocks = 0
    widths = np.zeros(1, np.int64)
    for Pg, Eg in proto:
        first = PG.envelope(len(Pg), Eg, 0 if ml else 2)[1]
        w = np.arange(len(first)) - first + 1
        blocks += int(w.sum())
        dense_blocks += len(first) ** 2
        h = np.bincount(w)
        widths = np.pad(widths, (0, max(0, len(h) - len(widths))))
        widths[:len(h)] += h
    edges_hist = [1, 2, 3, 4, 8, 16, 64, 256, 1024, 1 << 30]
    width_hist = {f"{lo}..{hi - 1}": int(widths[lo:hi].sum()) for lo, hi in zip(edges_hist[:-1], edges_hist[1:]) if widths[lo:hi].sum()}
    pg.optimise_flat(ranges, P, E, ml)                       # warm-up (workspace, code objects)
    walls, kern = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        _, status, chi2 = pg.optimise_flat(ranges, P, E, ml)
        walls.append(time.perf_counter() - t0)
    pg.set_timing(True)
    for _ in range(a.reps):
        pg.optimise_flat(ranges, P, E, ml)
        kern.append(pg.last_times()[0])
    launches = pg.last_times()[1]
    flops, lin_b, seg_b = pg.last_work()
    km = np.median(np.array(kern), 0)
    names = ["linearise", "assemble", "segment", "reduced", "backsub_update", "chi2", "full_call_device"]
    out = dict(graphs=a.graphs, frames=a.frames, keyframes=a.keyframes, loops=a.loops, schedule="multilevel" if ml else "single",
               reduced=a.reduced, envelope_blocks=blocks, dense_blocks=dense_blocks, envelope_row_widths=width_hist,
               device_ms_median=float(km[6]), wall_ms_median=1e3 * float(np.median(walls)), kernel_ms_median={n: float(x) for n, x in zip(names, km)}, launches=launches,
               status_ok=int((status == PG.OK).sum()),
               reduced_gflop=flops / 1e9, reduced_tflops=flops / (km[3] * 1e-3) / 1e12 if km[3] > 0 else None,
               reduced_fraction_of_fp64_vector_spec=flops / (km[3] * 1e-3) / (FP64_VECTOR_TFLOPS * 1e12) if km[3] > 0 else None,
               linearise_tbps=lin_b / (km[0] * 1e-3) / 1e12 if km[0] > 0 else None,
               segment_tbps=seg_b / ((km[1] + km[2] + km[4]) * 1e-3) / 1e12 if km[2] > 0 else None,
               hbm_spec_tbps=HBM_TBPS, chi2_ratio_median=float(np.median(chi2[:, 1] / chi2[:, 0])))
    pg.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
