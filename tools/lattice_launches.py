"""Launch times of the residual-lattice pre-pass by pyramid level, from a rocprofv3 --kernel-trace of bench.py (run on the GPU box).

  python tools/lattice_launches.py <dir> [--iters 10,5,3]

The lattice has the same 19 200 samples at every level of a 640 x 480 frame, so neither the kernel name nor the grid tells the levels apart; the
schedule does: a tracked step launches the kernel sum(iters) times, coarse to fine, so in time order the last iters[0] launches of every group are level 0.
Both variants of k_lattice_residuals_fused (<false>: fp32 maps, <true>: the raw input frame) are taken as one sequence and reported per variant and level."""
import argparse, collections, csv, glob, os
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("dir")
ap.add_argument("--iters", default="10,5,3", help="Gauss-Newton iterations of level 0, 1, 2, ... (the engine's default schedule)")
args = ap.parse_args()
iters = [int(v) for v in args.iters.split(",")]
order = [l for l in range(len(iters) - 1, -1, -1) for _ in range(iters[l])]   # level of the k-th lattice launch of a step

for tr in sorted(glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True)):
    rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(tr)) if "k_lattice_residuals_fused" in r["Kernel_Name"]]
    rows.sort()
    if not rows:
        continue
    print(f"{os.path.basename(tr)}: {len(rows)} lattice launches = {len(rows) / len(order):.2f} steps of {len(order)}")
    if len(rows) % len(order):
        print("  launch count is no multiple of the schedule: levels not assigned")
        continue
    agg = collections.defaultdict(list)
    for k, (t0, t1, name) in enumerate(rows):
        agg[("raw frame" if "<true>" in name else "fp32 maps", order[k % len(order)])].append((t1 - t0) * 1e-3)
    for (variant, level), v in sorted(agg.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        v = np.array(v)
        print(f"  level {level}  {variant:10s} launches {len(v):5d}  median {np.median(v):8.1f} us  mean {v.mean():8.1f}  min {v.min():8.1f}  max {v.max():8.1f}")
