#!/usr/bin/env python
"""How far two triangle meshes lie from each other (include/rgbid_meshdist.h): the distances of the vertices of A to
the surface of B and of the vertices of B to the surface of A, each truncated at --max-distance, as mean, rms, median, 90th percentile and
maximum over the vertices that found a triangle within that distance; the larger maximum is the vertex-sampled symmetric Hausdorff
distance, truncated.  Both files are PLYs as `track_dataset.py --mesh` writes them, in one frame -- or, with --register, in two: A is
first registered to B by point-to-plane ICP on its vertices (include/rgbid_meshreg.h), the pose and the status are
printed, and the distances are printed before and after.

    python tools/mesh_compare.py A.ply B.ply --max-distance D [--cell C] [--register [--starts identity|principal] [--out-aligned C.ply]]
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
    ap.add_argument("--register", action="store_true", help="register A to B first and print the pose, the status and the distances before and after")
    ap.add_argument("--starts", choices=("identity", "principal"), default=None,
                    help="with --register: start from the identity (the default) or from the four poses that match the principal axes")
    ap.add_argument("--out-aligned", default="", metavar="C.ply", help="with --register: write A, moved into B's frame, to C.ply")
    args = ap.parse_args()
    if args.max_distance is None:
        ap.error("--max-distance is required")
    if not args.register and (args.starts is not None or args.out_aligned):
        ap.error("--starts / --out-aligned need --register")
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
        (va, ca, ta, *na), (vb, _, tb, *_) = meshes
        if args.register:
            from rgbid import meshreg as MR
            reg = MR.register_mesh(ctx, dev(va), dev(ta), dev(vb), dev(tb), args.max_distance, args.starts or "identity", args.cell)
            figures = reg["after"]
            if args.out_aligned and reg["points"] is not None:
                moved, normals = reg["points"], None
                if na:
                    mover = MR.Registration(ctx, 1, 1, 1, 1, 1)
                    _, normals = mover.apply(dev(va), reg["R"], reg["t"], dev(na[0]))
                    mover.close()
                TS.write_mesh_ply(args.out_aligned, moved, ca, ta, normals)
        else:
            figures = MD.mesh_deviation(ctx, dev(va), dev(ta), dev(vb), dev(tb), args.max_distance, args.cell)
    except (ValueError, RuntimeError) as e:
        sys.exit(f"mesh_compare: {e}")
    finally:
        ctx.close()
    print(f"{args.a}: {len(va)} vertices, {len(ta)} triangles; {args.b}: {len(vb)} vertices, {len(tb)} triangles; truncated at {args.max_distance:g} m")
    if args.register:
        for line in MR.pose_lines(reg):
            print(line)
        print(f"before, A -> B: {MD.summary_line(reg['before']['a_to_b'])}")
        print(f"before, B -> A: {MD.summary_line(reg['before']['b_to_a'])}")
        if figures is None:
            sys.exit("mesh_compare: the registration found no pose")
        if args.out_aligned:
            print(f"A, moved into the frame of B, written to {args.out_aligned}")
        print("after:")
    print(f"A -> B: {MD.summary_line(figures['a_to_b'])}")
    print(f"B -> A: {MD.summary_line(figures['b_to_a'])}")
    print(f"vertex-sampled symmetric Hausdorff distance, truncated: {figures['hausdorff']:.6f} m")


if __name__ == "__main__":
    main()
