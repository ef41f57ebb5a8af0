#!/usr/bin/env python
"""How far two triangle meshes lie from each other (include/rgbid_meshdist.h): the distances of the vertices of A to
the surface of B and of the vertices of B to the surface of A, each truncated at --max-distance, as mean, rms, median, 90th percentile and
maximum over the vertices that found a triangle within that distance; the larger maximum is the vertex-sampled symmetric Hausdorff
distance, truncated.  Both files are PLYs as `track_dataset.py --mesh` writes them, in one frame.

    python tools/mesh_compare.py A.ply B.ply --max-distance D [--cell C]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rgbid-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a", metavar="A.ply")
    ap.add_argument("b", metavar="B.ply")
    ap.add_argument("--max-distance", type=float, default=None, metavar="D", help="the truncation distance in metres (required)")
    ap.add_argument("--cell", type=float, default=None, metavar="C", help="the edge of the search grid's cells in metres (default and minimum 1.0625 D)")
    args = ap.parse_args()
    if args.max_distance is None:
        ap.error("--max-distance is required")
    from rgbid import meshdist as MD
    from rgbid import tsdf as TS
    meshes = []
    try:
        MD.cell_arg(args.cell, MD.distance_arg(args.max_distance))
        for path in (args.a, args.b):
            try:
                with open(path, "rb") as f:
                    meshes.append(TS.read_mesh_ply(f.read()))
            except (OSError, ValueError, IndexError, UnicodeDecodeError) as e:
                raise ValueError(f"cannot read {path}: {e}") from None
    except ValueError as e:
        ap.error(str(e))
    import numpy as np
    import torch
    from rgbid import device
    if not torch.cuda.is_available():
        sys.exit("mesh_compare: needs a HIP device (there is no CPU path)")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x.view(np.int32) if x.dtype == np.uint32 else x)).cuda()
    ctx = device.Context(0)
    try:
        (va, _, ta, *_), (vb, _, tb, *_) = meshes
        figures = MD.mesh_deviation(ctx, dev(va), dev(ta), dev(vb), dev(tb), args.max_distance, args.cell)
    except (ValueError, RuntimeError) as e:
        sys.exit(f"mesh_compare: {e}")
    finally:
        ctx.close()
    print(f"{args.a}: {len(va)} vertices, {len(ta)} triangles; {args.b}: {len(vb)} vertices, {len(tb)} triangles; truncated at {args.max_distance:g} m")
    print(f"A -> B: {MD.summary_line(figures['a_to_b'])}")
    print(f"B -> A: {MD.summary_line(figures['b_to_a'])}")
    print(f"vertex-sampled symmetric Hausdorff distance, truncated: {figures['hausdorff']:.6f} m")


if __name__ == "__main__":
    main()
