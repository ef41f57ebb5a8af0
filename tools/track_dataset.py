#!/usr/bin/env python
"""Chunk-sharded tracking of a TUM / ICL-NUIM layout dataset with the batched engine (BASELINE config 4).

    python tools/track_dataset.py <dataset_folder> [--match-file f] [--chunks 8] [--out traj.txt] [--max-frames N]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 tools/track_dataset.py <folder> --chunks 8N

Frames are read with the product's own dataset reader (librgbid_host.so: association files, 16-bit PNG depth x0.2 -> mm), the
sequence is cut into `chunks` contiguous chunks with one frame of overlap, every chunk is one lane of a rank's engine, ranks exchange
the 392-byte per-frame records only (one all-gather over RCCL through librgbid_dist.so), rank 0 writes the trajectory in the TUM format (`stamp tx ty tz qx qy qz qw`)."""
import argparse
import os
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # before the HIP runtime comes up: the host driver only supports dmabuf IPC (RCCL across processes)
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rgbid-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch


def run_options(args):
    """the optimise / loops / loop_options / segment keywords of sequence.track_chunked that the parsed options ask for"""
    opt = dict(optimise=args.optimise, loops=args.loops) if args.optimise else {}
    lo = {}
    if args.loops == "appearance" and (args.loop_levels != 1 or args.loop_scale != 1.2):
        lo.update(levels=args.loop_levels, scale=args.loop_scale)
    if args.loop_proposal == "bow":
        lo.update(proposal="bow", vocabulary=args.loop_vocabulary)
        if args.loop_shortlist is not None:
            lo["shortlist_size"] = args.loop_shortlist
    if args.loop_mask_level:
        lo.update(mask_level=args.loop_mask_level, segment_k=args.segment_k, segment_min=args.segment_min, max_segments=args.segment_max)
    if lo:
        opt["loop_options"] = lo
    if args.labels_out:
        opt["segment"] = dict(k=args.segment_k, min_size=args.segment_min, max_segments=args.segment_max)
    return opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("folder")
    ap.add_argument("--match-file", default="")
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--out", default="trajectory.txt")
    ap.add_argument("--max-frames", type=int, default=-1)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--force-dist", action="store_true", help="initialise torch.distributed (RCCL) even with a single rank")
    ap.add_argument("--cloud", default="", metavar="PATH", help="also write the coloured point cloud of the exported keyframes as binary PLY "
                    "(the novel points, as the reference's viewer draws them); with several ranks each writes PATH with .rank<r> before the extension")
    ap.add_argument("--cloud-all", action="store_true", help="with --cloud: every valid pixel of every keyframe instead of the novel ones")
    ap.add_argument("--voxel", type=float, default=None, metavar="LEAF",
                    help="with --cloud: write the voxel-grid filtered map (centroids of LEAF-metre cells, as the reference writes its map: "
                    "0.01) instead of every point; with several ranks each rank filters its own points (voxels are not merged across ranks)")
    ap.add_argument("--cloud-radius", type=float, default=None, metavar="R",
                    help="with --cloud and --cloud-min-neighbours: first remove the isolated points, those with fewer than N other points of "
                    "the rank's cloud within R metres (DESIGN.md section 15); --voxel then filters what is left")
    ap.add_argument("--cloud-min-neighbours", type=int, default=None, metavar="N", help="with --cloud-radius: the neighbours a point needs to stay")
    ap.add_argument("--cloud-consistency", type=float, default=None, metavar="TOL_REL",
                    help="with --cloud: first remove the points that other keyframes saw through: a keyframe contradicts a point when, "
                         "along its own ray, it measured only depths more than TOL_REL x depth (+ --cloud-consistency-abs) behind it "
                         "(DESIGN.md section 18); --cloud-radius and --voxel then filter what is left; with --optimise the optimised poses are used")
    ap.add_argument("--cloud-consistency-abs", type=float, default=None, metavar="M", help="with --cloud-consistency: metres added to the tolerance (default 0)")
    ap.add_argument("--cloud-consistency-window", type=int, default=None, metavar="W",
                    help="with --cloud-consistency: a keyframe looks at the (2 W + 1)^2 pixels around the point's projection (0 .. 2, default 1)")
    ap.add_argument("--cloud-min-support", type=int, default=None, metavar="S",
                    help="with --cloud-consistency: other keyframes that must have measured the point's depth for it to stay (default 0)")
    ap.add_argument("--cloud-max-conflicts", type=int, default=None, metavar="C",
                    help="with --cloud-consistency: contradicting keyframes a point may have and stay (default 0)")
    ap.add_argument("--render", default="", metavar="DIR",
                    help="with --cloud: render the map that --cloud writes (after --cloud-radius and --voxel) at every exported keyframe's "
                         "pose on the device and write DIR/view_<i>.png (colour) and DIR/view_<i>_depth.png (16-bit, metres x 5000 as TUM "
                         "depth files are scaled, 0 where the map is empty); DESIGN.md section 17")
    ap.add_argument("--render-splat", type=int, default=None, metavar="S",
                    help="with --render / --render-check: every point paints the (2 S + 1)^2 pixels around its own (0 .. 4, default 1)")
    ap.add_argument("--render-check", action="store_true",
                    help="with --cloud: print how well the keyframe cloud, rendered at each keyframe's pose without the keyframe's own points, "
                         "agrees with the depth that keyframe measured (pixels compared, median and 90th percentile of the difference in "
                         "metres), per keyframe and over the run; with --optimise before and after the optimisation.  It reads the cloud "
                         "before --cloud-radius and --voxel: only there does a point still belong to its keyframe")
    ap.add_argument("--mesh", default="", metavar="PATH",
                    help="fuse the exported keyframes' depth and colours into a TSDF volume on the device and write its surface as a binary "
                         "PLY triangle mesh (DESIGN.md section 19); with --optimise the optimised poses are used; with several ranks each "
                         "writes PATH with .rank<r> before the extension")
    ap.add_argument("--mesh-voxel", type=float, default=None, metavar="H", help="with --mesh: the voxel size in metres (default 0.02)")
    ap.add_argument("--mesh-trunc", type=float, default=None, metavar="T", help="with --mesh: the truncation distance in metres (default 4 H)")
    ap.add_argument("--mesh-min-weight", type=int, default=None, metavar="W",
                    help="with --mesh: keyframes that must have measured a voxel for the surface to pass it (1 .. 65535, default 1)")
    ap.add_argument("--mesh-bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                    help="with --mesh: the volume's box in world metres (default: the box of the keyframe cloud, padded by T)")
    ap.add_argument("--mesh-max-voxels", type=int, default=None, metavar="N", help="with --mesh: the largest volume to allocate (default 2^27 voxels)")
    ap.add_argument("--mesh-min-component", type=int, default=None, metavar="N",
                    help="with --mesh: drop the connected components of the mesh with fewer than N triangles (DESIGN.md section 22)")
    ap.add_argument("--mesh-largest-components", type=int, default=None, metavar="K",
                    help="with --mesh: keep only the K connected components of the mesh with the most triangles")
    ap.add_argument("--mesh-simplify", type=float, default=None, metavar="CELL",
                    help="with --mesh: decimate the mesh by vertex clustering with cells of CELL metres (DESIGN.md section 23); after the "
                         "component options when both are given")
    ap.add_argument("--mesh-fill-holes", type=int, default=None, metavar="N",
                    help="with --mesh: close the loops of at most N boundary edges by a fan around a new vertex each (DESIGN.md section 30), "
                         "after the component and simplify options and before --mesh-smooth")
    ap.add_argument("--mesh-fill-any-facing", action="store_true",
                    help="with --mesh-fill-holes: also close the loops whose cap would face against their rim's triangles (the outer edges of fragments)")
    ap.add_argument("--mesh-refine", type=float, default=None, metavar="L",
                    help="with --mesh: split the edges of the mesh that are longer than L metres at their midpoints until none is left or the "
                         "rounds run out (DESIGN.md section 33), after the component, simplify and fill options and before --mesh-denoise and "
                         "--mesh-smooth")
    ap.add_argument("--mesh-refine-rounds", type=int, default=None, metavar="R",
                    help="with --mesh-refine: the most rounds, each of which halves the edges that are too long, 0 .. 16 (default 4)")
    ap.add_argument("--mesh-refine-caps", action="store_true",
                    help="with --mesh-refine and --mesh-fill-holes: split only the fans that closed the holes, and the neighbours that share a split rim edge")
    ap.add_argument("--mesh-denoise", type=int, default=None, metavar="N",
                    help="with --mesh: denoise the mesh with its sharp edges kept, N iterations over the face normals (0 .. 256; DESIGN.md section 32), "
                         "after the component, simplify and fill options and before --mesh-smooth; with --mesh-normals the normals are those of the "
                         "denoised surface")
    ap.add_argument("--mesh-denoise-vertex-iterations", type=int, default=None, metavar="M",
                    help="with --mesh-denoise: the passes that move the vertices along the filtered normals, 0 .. 256 (default 10)")
    ap.add_argument("--mesh-denoise-threshold", type=float, default=None, metavar="T",
                    help="with --mesh-denoise: a face hears a neighbour only where the dot product of their normals exceeds T, 0 <= T < 1 (default 0.4)")
    ap.add_argument("--mesh-smooth", type=int, default=None, metavar="N",
                    help="with --mesh: move the vertices by N iterations of Taubin's filter (DESIGN.md section 24), after the component and "
                         "simplify options; with --mesh-normals the normals are those of the smoothed surface")
    ap.add_argument("--mesh-smooth-lambda", type=float, default=None, metavar="L", help="with --mesh-smooth: the positive factor, 0 < L <= 1 (default 0.5)")
    ap.add_argument("--mesh-smooth-mu", type=float, default=None, metavar="M",
                    help="with --mesh-smooth: the negative factor, -2 <= M <= 0 (default -0.53; 0: plain Laplacian smoothing)")
    ap.add_argument("--mesh-smooth-pin-boundary", action="store_true", help="with --mesh-smooth: the vertices on a boundary of the mesh do not move")
    ap.add_argument("--mesh-normals", action="store_true", help="with --mesh: the PLY also holds a unit normal per vertex (nx ny nz)")
    ap.add_argument("--mesh-render", default="", metavar="DIR",
                    help="with --mesh: ray-cast the fused volume at every exported keyframe's pose (DESIGN.md section 20) and write "
                         "view_NNNN.png (colour), view_NNNN_depth.png (16-bit, metres * 5000) and view_NNNN_shaded.png into DIR")
    ap.add_argument("--mesh-render-check", action="store_true",
                    help="with --mesh: print how well the fused surface, ray-cast at each keyframe's pose, agrees with the depth the keyframe measured")
    ap.add_argument("--mesh-render-step", type=float, default=None, metavar="S",
                    help="with --mesh-render / --mesh-render-check: metres of camera depth between two samples of a ray (default: the voxel size)")
    ap.add_argument("--mesh-raster", default="", metavar="DIR",
                    help="with --mesh: rasterise the mesh that is written, after all clean-up options, at every exported keyframe's pose "
                         "(DESIGN.md section 25) and write mesh_NNNN.png (colour), mesh_NNNN_depth.png (16-bit, metres x 5000, empty = 0) and, with "
                         "--mesh-normals, mesh_NNNN_shaded.png into DIR")
    ap.add_argument("--mesh-raster-check", action="store_true",
                    help="with --mesh: print how well the written mesh, rasterised at each keyframe's pose, agrees with the depth the keyframe measured")
    ap.add_argument("--mesh-deviation", type=float, default=None, metavar="D",
                    help="with --mesh and at least one of --mesh-min-component / --mesh-largest-components / --mesh-simplify / --mesh-smooth: print how far "
                         "the written mesh lies from the mesh as extracted, without those options, and the other way round (DESIGN.md section 26): "
                         "the distances of the vertices of one to the surface of the other, truncated at D metres")
    ap.add_argument("--mesh-reference", default="", metavar="MODEL.ply",
                    help="with --mesh: print how far the written mesh lies from the triangle mesh MODEL.ply (a PLY as --mesh writes it, in the "
                         "world frame) and the other way round")
    ap.add_argument("--mesh-reference-distance", type=float, default=None, metavar="D",
                    help="with --mesh-reference: the truncation distance in metres (default: the volume's truncation distance)")
    ap.add_argument("--mesh-reference-register", action="store_true",
                    help="with --mesh-reference: first register the written mesh to MODEL.ply by point-to-plane ICP from the identity (DESIGN.md "
                         "section 28), print the pose and the status, and print the distances before and after; the written file is not moved")
    ap.add_argument("--mesh-recolour", choices=("mean", "best"), default=None,
                    help="with --mesh: recolour the vertices of the mesh that is written, after all clean-up options, from the keyframes that see "
                         "them, sampled at full resolution (DESIGN.md section 27): the weighted mean of those keyframes, or the one that faces "
                         "the vertex most")
    ap.add_argument("--mesh-recolour-tolerance", type=float, default=None, metavar="M",
                    help="with --mesh-recolour: metres between a vertex and the mesh's own depth in a keyframe for the keyframe to see it (default 2 H)")
    ap.add_argument("--mesh-recolour-measured", type=float, default=None, metavar="M",
                    help="with --mesh-recolour: also ask that the keyframe's own depth lies within M metres of the vertex")
    ap.add_argument("--mesh-colour-align", action="store_true",
                    help="with --mesh-recolour or --mesh-texture: refine the keyframes' poses against the mesh's colours first (colour map optimisation, "
                         "rigid part: DESIGN.md section 31); the geometry stays as it is, only the colours are sampled at the refined poses")
    ap.add_argument("--mesh-colour-align-scales", default=None, metavar="F,F,...", help="with --mesh-colour-align: the coarse-to-fine factors (default 4,2,1)")
    ap.add_argument("--mesh-colour-align-rounds", type=int, default=None, metavar="N", help="with --mesh-colour-align: target passes per scale (default 4)")
    ap.add_argument("--mesh-colour-align-fixed", choices=("first", "none"), default=None,
                    help="with --mesh-colour-align: hold the first keyframe's pose (the default) or none")
    ap.add_argument("--mesh-texture", default="", metavar="OUT.obj",
                    help="with --mesh: also write the mesh that is written, after all clean-up options, as OUT.obj with OUT.mtl and the texture "
                         "atlas OUT.png: every triangle gets a patch of an image baked from the keyframes that see it, sampled at full "
                         "resolution (DESIGN.md section 29); texels no keyframe sees are filled from the vertex colours")
    ap.add_argument("--mesh-texture-patch", type=int, default=None, metavar="N", help="with --mesh-texture: texels along a leg of a triangle's patch (2 .. 30, default 6)")
    ap.add_argument("--mesh-texture-mode", choices=("mean", "best"), default=None,
                    help="with --mesh-texture: the weighted mean of the keyframes that see a texel (the default), or the one that faces it most")
    ap.add_argument("--mesh-texture-tolerance", type=float, default=None, metavar="M",
                    help="with --mesh-texture: metres between a texel and the mesh's own depth in a keyframe for the keyframe to see it (default 2 H)")
    ap.add_argument("--mesh-texture-measured", type=float, default=None, metavar="M",
                    help="with --mesh-texture: also ask that the keyframe's own depth lies within M metres of the texel")
    ap.add_argument("--mesh-align-check", action="store_true",
                    help="with --mesh: fuse the even-numbered keyframes, align the odd-numbered ones to that model (DESIGN.md section 21) and print "
                         "the corrections the alignment proposes; nothing is applied")
    ap.add_argument("--mesh-align-iterations", type=int, default=None, metavar="N",
                    help="with --mesh-align-check: Gauss-Newton iterations per level of the strides 4, 2, 1 (1 .. 85, default 10)")
    ap.add_argument("--optimise", nargs="?", const="auto", default=None, choices=["auto", "multilevel", "single"],
                    help="optimise the trajectory with the pose-graph back-end once over the run (single rank; DESIGN.md section 11)")
    ap.add_argument("--loops", default=None, choices=["auto", "appearance"],
                    help="with --optimise: add loop constraints from the dense keyframe verifier; auto: candidates by distance on the trajectory, "
                         "appearance: by binary features, Hamming matching and RANSAC (DESIGN.md section 13)")
    ap.add_argument("--loop-levels", type=int, default=1, metavar="N",
                    help="with --loops appearance: extract the features over a pyramid of N levels (1 .. 8; the reference uses 8), so that a "
                         "revisit at another distance still matches")
    ap.add_argument("--loop-scale", type=float, default=1.2, metavar="S", help="with --loop-levels: the scale between neighbouring levels (1 < S <= 2)")
    ap.add_argument("--loop-proposal", default=None, choices=["match", "bow"],
                    help="with --loops appearance: match every keyframe pair (match, the default) or only the candidates a binary vocabulary "
                         "shortlists per keyframe (bow; DESIGN.md section 14)")
    ap.add_argument("--loop-vocabulary", default=None, metavar="FILE",
                    help="with --loop-proposal bow: load the vocabulary from FILE if it exists, otherwise train it on this run and save it there")
    ap.add_argument("--loop-shortlist", type=int, default=None, metavar="T", help="with --loop-proposal bow: candidates kept per keyframe (default 8)")
    ap.add_argument("--loop-mask-level", type=int, default=0, metavar="M",
                    help="with --loops appearance: match only the keypoints that negentropy mask M (1 .. 3) of their keyframe keeps, which takes "
                         "the features off large low-information surfaces (DESIGN.md section 16); 0: every keypoint")
    ap.add_argument("--segment-k", type=float, default=None, metavar="K", help="the segmenter's threshold constant (default 0.6)")
    ap.add_argument("--segment-min", type=int, default=None, metavar="N", help="the segmenter's smallest segment in points (default 300)")
    ap.add_argument("--segment-max", type=int, default=None, metavar="S",
                    help="segments per keyframe the segmenter's tables start with (default 4096; a keyframe with more is segmented again "
                         "with tables of its count)")
    ap.add_argument("--labels-out", default="", metavar="DIR",
                    help="segment every exported keyframe of this rank and write its labels as DIR/labels_<chunk>_<export>.npy (int32 "
                         "[rows, cols], -1 where the pixel is no point)")
    ap.add_argument("--K", type=float, nargs=4, default=[525.0, 525.0, 319.5, 239.5], help="fx fy cx cy (tools/evaluation.cpp:64-67)")
    args = ap.parse_args()
    if args.voxel is not None and not args.cloud:
        ap.error("--voxel needs --cloud")
    if args.render and not args.cloud:
        ap.error("--render needs --cloud")
    if args.render_check and not args.cloud:
        ap.error("--render-check needs --cloud")
    if args.render_splat is not None and not (args.render or args.render_check):
        ap.error("--render-splat needs --render or --render-check")
    if args.render or args.render_check:
        from rgbid import render as RD
        try:
            splat = RD.splat_arg(1 if args.render_splat is None else args.render_splat)
        except ValueError as e:
            ap.error(str(e))
    if args.cloud_consistency is not None and not args.cloud:
        ap.error("--cloud-consistency needs --cloud")
    if args.cloud_consistency is None and not (args.cloud_consistency_abs is None and args.cloud_consistency_window is None
                                               and args.cloud_min_support is None and args.cloud_max_conflicts is None):
        ap.error("--cloud-consistency-abs / --cloud-consistency-window / --cloud-min-support / --cloud-max-conflicts need --cloud-consistency")
    if args.cloud_consistency is not None:
        from rgbid import consist as CF
        try:
            consist = dict(zip(("tol_rel", "tol_abs"), CF.tolerances(args.cloud_consistency, args.cloud_consistency_abs or 0.0)))
            consist["window"] = CF.window_arg(1 if args.cloud_consistency_window is None else args.cloud_consistency_window)
            consist.update(zip(("min_support", "max_conflicts"), CF.vote_args(args.cloud_min_support or 0, args.cloud_max_conflicts or 0)))
        except ValueError as e:
            ap.error(str(e))
    if not args.mesh and not (args.mesh_voxel is None and args.mesh_trunc is None and args.mesh_min_weight is None and args.mesh_bounds is None
                              and args.mesh_max_voxels is None):
        ap.error("--mesh-voxel / --mesh-trunc / --mesh-min-weight / --mesh-bounds / --mesh-max-voxels need --mesh")
    if not args.mesh and (args.mesh_normals or args.mesh_render or args.mesh_render_check or args.mesh_render_step is not None):
        ap.error("--mesh-normals / --mesh-render / --mesh-render-check / --mesh-render-step need --mesh")
    if args.mesh_render_step is not None and not (args.mesh_render or args.mesh_render_check):
        ap.error("--mesh-render-step needs --mesh-render or --mesh-render-check")
    if not args.mesh and (args.mesh_raster or args.mesh_raster_check):
        ap.error("--mesh-raster / --mesh-raster-check need --mesh")
    if not args.mesh and args.mesh_recolour is not None:
        ap.error("--mesh-recolour needs --mesh")
    if args.mesh_recolour is None and (args.mesh_recolour_tolerance is not None or args.mesh_recolour_measured is not None):
        ap.error("--mesh-recolour-tolerance / --mesh-recolour-measured need --mesh-recolour")
    if not args.mesh and args.mesh_texture:
        ap.error("--mesh-texture needs --mesh")
    if args.mesh_colour_align and args.mesh_recolour is None and not args.mesh_texture:
        ap.error("--mesh-colour-align needs --mesh-recolour or --mesh-texture")
    if not args.mesh_colour_align and (args.mesh_colour_align_scales is not None or args.mesh_colour_align_rounds is not None
                                       or args.mesh_colour_align_fixed is not None):
        ap.error("--mesh-colour-align-scales / --mesh-colour-align-rounds / --mesh-colour-align-fixed need --mesh-colour-align")
    if not args.mesh_texture and (args.mesh_texture_patch is not None or args.mesh_texture_mode is not None or args.mesh_texture_tolerance is not None
                                  or args.mesh_texture_measured is not None):
        ap.error("--mesh-texture-patch / --mesh-texture-mode / --mesh-texture-tolerance / --mesh-texture-measured need --mesh-texture")
    if not args.mesh and (args.mesh_align_check or args.mesh_align_iterations is not None):
        ap.error("--mesh-align-check / --mesh-align-iterations need --mesh")
    if args.mesh_align_iterations is not None and not args.mesh_align_check:
        ap.error("--mesh-align-iterations needs --mesh-align-check")
    if not args.mesh and (args.mesh_min_component is not None or args.mesh_largest_components is not None):
        ap.error("--mesh-min-component / --mesh-largest-components need --mesh")
    if not args.mesh and args.mesh_simplify is not None:
        ap.error("--mesh-simplify needs --mesh")
    if not args.mesh and args.mesh_fill_holes is not None:
        ap.error("--mesh-fill-holes needs --mesh")
    if args.mesh_fill_holes is None and args.mesh_fill_any_facing:
        ap.error("--mesh-fill-any-facing needs --mesh-fill-holes")
    if not args.mesh and args.mesh_refine is not None:
        ap.error("--mesh-refine needs --mesh")
    if args.mesh_refine is None and (args.mesh_refine_rounds is not None or args.mesh_refine_caps):
        ap.error("--mesh-refine-rounds / --mesh-refine-caps need --mesh-refine")
    if args.mesh_refine_caps and args.mesh_fill_holes is None:
        ap.error("--mesh-refine-caps needs --mesh-fill-holes")
    if not args.mesh and args.mesh_denoise is not None:
        ap.error("--mesh-denoise needs --mesh")
    if args.mesh_denoise is None and (args.mesh_denoise_vertex_iterations is not None or args.mesh_denoise_threshold is not None):
        ap.error("--mesh-denoise-vertex-iterations / --mesh-denoise-threshold need --mesh-denoise")
    if not args.mesh and args.mesh_smooth is not None:
        ap.error("--mesh-smooth needs --mesh")
    if args.mesh_smooth is None and (args.mesh_smooth_lambda is not None or args.mesh_smooth_mu is not None or args.mesh_smooth_pin_boundary):
        ap.error("--mesh-smooth-lambda / --mesh-smooth-mu / --mesh-smooth-pin-boundary need --mesh-smooth")
    if not args.mesh and (args.mesh_deviation is not None or args.mesh_reference or args.mesh_reference_distance is not None):
        ap.error("--mesh-deviation / --mesh-reference / --mesh-reference-distance need --mesh")
    if args.mesh_reference_distance is not None and not args.mesh_reference:
        ap.error("--mesh-reference-distance needs --mesh-reference")
    if args.mesh_reference_register and not args.mesh_reference:
        ap.error("--mesh-reference-register needs --mesh-reference")
    if args.mesh_deviation is not None and (args.mesh_min_component is None and args.mesh_largest_components is None and args.mesh_simplify is None
                                            and args.mesh_smooth is None):
        ap.error("--mesh-deviation needs at least one of --mesh-min-component / --mesh-largest-components / --mesh-simplify / --mesh-smooth")
    mesh_filter = {}
    if args.mesh:
        from rgbid import tsdf as TS
        try:
            mesh = dict(voxel=0.02 if args.mesh_voxel is None else args.mesh_voxel, min_weight=TS.weight_arg(1 if args.mesh_min_weight is None else args.mesh_min_weight))
            mesh["trunc"] = 4.0 * mesh["voxel"] if args.mesh_trunc is None else args.mesh_trunc
            mesh["max_voxels"] = TS.capacity_arg((1 << 27) if args.mesh_max_voxels is None else args.mesh_max_voxels, 1)[0]
            TS.grid_arg(2, 2, 2, (0.0, 0.0, 0.0), mesh["voxel"], mesh["trunc"])
            if args.mesh_bounds is not None:
                TS.bounds_grid(args.mesh_bounds, mesh["voxel"], mesh["max_voxels"])
                mesh["bounds"] = args.mesh_bounds
            if args.mesh_render_step is not None:
                TS.step_arg(args.mesh_render_step, 0.05, 20.0)
            if args.mesh_align_check:
                n_it = 10 if args.mesh_align_iterations is None else args.mesh_align_iterations
                align_levels = TS.align_levels_arg(tuple((s, n_it) for s in (4, 2, 1)))
            if TS.component_filter_arg(args.mesh_min_component, args.mesh_largest_components) is not None:
                mesh_filter = dict(min_component=args.mesh_min_component, largest_components=args.mesh_largest_components)
            if TS.simplify_arg(args.mesh_simplify) is not None:
                mesh_filter["simplify"] = args.mesh_simplify
            if args.mesh_fill_holes is not None:
                from rgbid import holes as HO
                mesh_filter["fill_holes"] = HO.fill_holes_arg(dict(max_edges=args.mesh_fill_holes, any_facing=args.mesh_fill_any_facing))
            if args.mesh_refine is not None:
                from rgbid import refine as RF
                mesh_filter["refine"] = RF.refine_arg(dict(max_edge=args.mesh_refine, rounds=4 if args.mesh_refine_rounds is None else args.mesh_refine_rounds,
                                                           caps_only=args.mesh_refine_caps))
            if args.mesh_denoise is not None:
                from rgbid import denoise as DN
                mesh_filter["denoise"] = DN.denoise_arg(dict(normal_iterations=args.mesh_denoise,
                                                             vertex_iterations=10 if args.mesh_denoise_vertex_iterations is None else args.mesh_denoise_vertex_iterations,
                                                             threshold=0.4 if args.mesh_denoise_threshold is None else args.mesh_denoise_threshold))
            if args.mesh_smooth is not None:
                mesh_filter["smooth"] = TS.smooth_arg(dict(iterations=args.mesh_smooth, lam=0.5 if args.mesh_smooth_lambda is None else args.mesh_smooth_lambda,
                                                           mu=-0.53 if args.mesh_smooth_mu is None else args.mesh_smooth_mu,
                                                           pin_boundary=args.mesh_smooth_pin_boundary))
            if args.mesh_recolour is not None:
                from rgbid import recolour as RC
                mesh_filter["recolour"] = args.mesh_recolour
                if args.mesh_recolour_tolerance is not None:
                    mesh_filter["recolour_tolerance"] = RC.tolerance_arg("--mesh-recolour-tolerance", args.mesh_recolour_tolerance)
                if args.mesh_recolour_measured is not None:
                    mesh_filter["recolour_measured"] = RC.tolerance_arg("--mesh-recolour-measured", args.mesh_recolour_measured)
            if args.mesh_colour_align:
                from rgbid import colouralign as CA
                try:
                    scales = (4, 2, 1) if args.mesh_colour_align_scales is None else tuple(int(f) for f in args.mesh_colour_align_scales.split(","))
                except ValueError:
                    ap.error(f"--mesh-colour-align-scales: integers separated by commas, got {args.mesh_colour_align_scales!r}")
                mesh_filter["colour_align"] = dict(scales=CA.scales_arg(scales, args.rows, args.cols),
                                                   rounds=4 if args.mesh_colour_align_rounds is None else args.mesh_colour_align_rounds,
                                                   fixed=None if args.mesh_colour_align_fixed == "none" else (0,))
                CA.rule_arg(16.0, 0.0, 1e-7, 6, 2, mesh_filter["colour_align"]["rounds"], 3, 1)
            texture = None
            if args.mesh_texture:
                from rgbid import recolour as RC
                from rgbid import texture as TX
                TX.obj_paths(args.mesh_texture)
                texture = dict(patch=TX.patch_arg(6 if args.mesh_texture_patch is None else args.mesh_texture_patch), mode=args.mesh_texture_mode or "mean",
                               surface_tolerance=RC.tolerance_arg("--mesh-texture-tolerance", 2.0 * mesh["voxel"] if args.mesh_texture_tolerance is None
                                                                  else args.mesh_texture_tolerance))
                if args.mesh_texture_measured is not None:
                    texture["measured_tolerance"] = RC.tolerance_arg("--mesh-texture-measured", args.mesh_texture_measured)
            reference = None
            if args.mesh_deviation is not None or args.mesh_reference:
                from rgbid import meshdist as MD
                if args.mesh_deviation is not None:
                    MD.distance_arg(args.mesh_deviation)
                if args.mesh_reference:
                    reference_distance = MD.distance_arg(mesh["trunc"] if args.mesh_reference_distance is None else args.mesh_reference_distance)
                    try:
                        with open(args.mesh_reference, "rb") as f:
                            reference = TS.read_mesh_ply(f.read())
                    except (OSError, ValueError, IndexError, UnicodeDecodeError) as e:
                        raise ValueError(f"--mesh-reference: cannot read {args.mesh_reference}: {e}") from None
        except ValueError as e:
            ap.error(str(e))
    if (args.cloud_radius is None) != (args.cloud_min_neighbours is None):
        ap.error("--cloud-radius and --cloud-min-neighbours need each other")
    if args.cloud_radius is not None:
        if not args.cloud:
            ap.error("--cloud-radius / --cloud-min-neighbours need --cloud")
        from rgbid import outlier as OL
        try:
            OL.radius32(args.cloud_radius); OL.neighbour_args(args.cloud_min_neighbours)
        except ValueError as e:
            ap.error(str(e))

    world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0")); local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path)"
    torch.cuda.set_device(local_rank)
    use_dist = world > 1 or args.force_dist
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    from rgbid import device, sequence, tum

    ds = tum.Dataset(args.folder, args.match_file)
    n = len(ds) if args.max_frames < 0 else min(len(ds), args.max_frames)
    frames, stamps = [], []
    for k in range(n):
        g = ds.grab(k, args.rows, args.cols)
        if g is None:                      # unreadable pair: the reference's playback skips it too
            continue
        frames.append(g); stamps.append(ds.stamp(k))
    assert len(frames) >= args.chunks + 1, "need at least chunks + 1 readable frames"
    depth = torch.from_numpy(np.stack([f[0] for f in frames]).view(np.int16)).cuda()
    rgb = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    ctx = device.Context(local_rank)
    ctx.set_async(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    comm = None
    if use_dist:
        from rgbid import dist as D
        try:
            comm = D.Comm(ctx, world, rank)          # the C-ABI RCCL helper (librgbid_dist.so); the id travels through torch's store
        except Exception as e:                       # transport problem: say so, gather through torch.distributed instead
            sys.stderr.write(f"[track_dataset] WARNING: C-ABI RCCL communicator failed ({e}); gathering through torch.distributed\n")
    if args.loops and not args.optimise:
        ap.error("--loops needs --optimise")
    if (args.loop_levels != 1 or args.loop_scale != 1.2) and args.loops != "appearance":
        ap.error("--loop-levels / --loop-scale need --loops appearance")
    if (args.loop_proposal is not None or args.loop_vocabulary is not None or args.loop_shortlist is not None) and args.loops != "appearance":
        ap.error("--loop-proposal / --loop-vocabulary / --loop-shortlist need --loops appearance")
    if (args.loop_vocabulary is not None or args.loop_shortlist is not None) and args.loop_proposal != "bow":
        ap.error("--loop-vocabulary / --loop-shortlist need --loop-proposal bow")
    if args.loop_mask_level and args.loops != "appearance":
        ap.error("--loop-mask-level needs --loops appearance")
    if not 0 <= args.loop_mask_level <= 3:
        ap.error("--loop-mask-level must lie in 0 .. 3")
    if (args.segment_k is not None or args.segment_min is not None or args.segment_max is not None) and not (args.loop_mask_level or args.labels_out):
        ap.error("--segment-k / --segment-min / --segment-max need --loop-mask-level or --labels-out")
    opt = run_options(args)
    if args.render_check or args.cloud_consistency is not None:
        opt["keyframe_depth"] = True
    if args.mesh:
        opt.update(keyframe_depth=True, keyframe_colour=True)
    if args.cloud or args.mesh:
        R, t, ranges, pc = sequence.track_chunked(ctx, depth, rgb, args.chunks, tuple(args.K), comm=comm, use_graph=0,
                                                  cloud="all" if args.cloud_all else "novel", **opt)
    else:
        R, t, ranges = sequence.track_chunked(ctx, depth, rgb, args.chunks, tuple(args.K), comm=comm, use_graph=0, **opt)
    if args.optimise:
        info = sequence.track_chunked.last_optimise
        print(f"pose graph: {info['mode']}, status {info['status']}, chi2 {info['chi2'][0]:.4g} -> {info['chi2'][1]:.4g}, "
              f"loops accepted {info['accepted']} of {len(info['loops'])}")
        for a in info.get("appearance", []):
            print(f"  appearance pair {a['query']} <- {a['candidate']}: score {a['score']:.3f}, matches {a['matches']}, inliers {a['inliers']}, "
                  f"hull {a['hull_query']:.3f} / {a['hull_candidate']:.3f}, ransac {'ok' if a['ransac_ok'] else 'refused'}"
                  + (f", bow score {a['bow_score']:.3f} rank {a['bow_rank']}" if "bow_rank" in a else ""))
    el = time.perf_counter() - t0
    if args.labels_out:
        os.makedirs(args.labels_out, exist_ok=True)
        for chunk, seq, labels in sequence.track_chunked.last_labels:
            np.save(os.path.join(args.labels_out, f"labels_{chunk:04d}_{seq:04d}.npy"), labels)
        print(f"rank {rank}: labels of {len(sequence.track_chunked.last_labels)} keyframes -> {args.labels_out}")
    if args.cloud:
        from rgbid import cloud as CL
        path = args.cloud
        if world > 1:
            root, ext = os.path.splitext(path)
            path = f"{root}.rank{rank}{ext}"
        points, said = pc.points, f"rank {rank}: {len(pc)} points of {len(pc.keyframes)} keyframes"
        consistent = None
        if args.cloud_consistency is not None and pc.keyframes:
            points, kept_offsets, cp = CF.consistency_filter(ctx, points, pc.offsets, [k["depthinv"] for k in pc.keyframes],
                                                             np.stack([k["R"] for k in pc.keyframes]), np.stack([k["t"] for k in pc.keyframes]),
                                                             tuple(args.K), args.rows, args.cols, return_offsets=True, return_plan=True, **consist)
            consistent = (points, kept_offsets)
            said += (f" -> {cp.kept} kept, {cp.n - cp.kept} removed, {cp.contradicted} contradicted (tolerance {consist['tol_rel']:g} x depth"
                     f" + {consist['tol_abs']:g} m, window {consist['window']}, support >= {consist['min_support']}, conflicts <= {consist['max_conflicts']})")
        after_consistency = points.shape[0]
        if args.cloud_radius is not None:
            points = OL.radius_filter(ctx, points, args.cloud_radius, args.cloud_min_neighbours)
            said += f" -> {points.shape[0]} kept of {after_consistency} ({args.cloud_min_neighbours} within {args.cloud_radius:g} m)"
        if args.voxel is None:
            CL.write_ply(path, points)
            print(f"{said} -> {path}")
        else:
            from rgbid import voxel as VX
            vox, plan = VX.voxel_grid(ctx, points, args.voxel, return_plan=True)
            CL.write_ply(path, vox)
            print(f"{said} -> {plan.voxels} voxels of {args.voxel:g} m -> {path}")
            points = vox
        if args.render_check:
            clouds = [("", pc)]
            if args.optimise:
                clouds = [(" before the optimisation", sequence.track_chunked.last_cloud_before), (" after the optimisation", pc)]
            if consistent is not None:
                clouds.append((" after the consistency filter", CL.ChunkCloud(consistent[0], consistent[1], pc.keyframes)))
            for when, c in clouds:
                figures = RD.depth_agreement(ctx, c.points, c.offsets, c.keyframes, tuple(args.K), args.rows, args.cols, splat)
                for kf, f in zip(c.keyframes, figures):
                    print(f"rank {rank}: render check{when}: keyframe at frame {kf['frame']}: {f['pixels']} pixels, "
                          f"median {f['median']:.6f} m, 90 % {f['p90']:.6f} m")
                run = RD.agreement_summary(figures)
                print(f"rank {rank}: render check{when}: {len(figures)} keyframes, {run['pixels']} pixels, median of medians {run['median']:.6f} m, "
                      f"largest 90 % {run['p90']:.6f} m")
        if args.render:
            os.makedirs(args.render, exist_ok=True)
            for a in range(0, len(pc.keyframes), RD.VIEW_CHUNK):
                kfs = pc.keyframes[a:a + RD.VIEW_CHUNK]
                views = RD.render_views(ctx, points, np.stack([k["R"] for k in kfs]), np.stack([k["t"] for k in kfs]), tuple(args.K), args.rows,
                                        args.cols, splat)
                for j in range(len(kfs)):
                    name = f"view_{a + j:04d}" if world == 1 else f"view_rank{rank}_{a + j:04d}"
                    tum.write_png(os.path.join(args.render, name + ".png"), views["colour"][j].cpu().numpy())
                    tum.write_png(os.path.join(args.render, name + "_depth.png"), RD.depth_png(views["depth"][j]))
            print(f"rank {rank}: {len(pc.keyframes)} views of {points.shape[0]} records, splat {splat} -> {args.render}")
    if args.mesh:
        path = args.mesh
        if world > 1:
            root, ext = os.path.splitext(path)
            path = f"{root}.rank{rank}{ext}"
        if not pc.keyframes:
            sys.exit(f"rank {rank}: --mesh: the run exported no keyframe")
        cast = bool(args.mesh_render or args.mesh_render_check)
        keep = cast or args.mesh_deviation is not None          # the deviation extracts the volume once more, without the clean-up options
        try:
            fused = TS.fuse(ctx, pc.keyframes, tuple(args.K), args.rows, args.cols, points=pc.points, return_volume=True, normals=args.mesh_normals,
                            keep_volume=keep, **mesh, **mesh_filter)
        except ValueError as e:
            sys.exit(f"rank {rank}: --mesh: {e}")
        verts, cols, tris = fused[:3]
        vol = fused[4 if args.mesh_normals else 3]
        TS.write_mesh_ply(path, verts, cols, tris, fused[3] if args.mesh_normals else None)
        flt = vol.get("filter")             # the line below tells the extraction's counts, the one after it what the filter left
        simp = vol.get("simplify")          # ... and the third what the decimation made of that
        fil = vol.get("fill_holes")         # ... and what the filling added is no part of the extraction's counts either
        first = flt or (dict(vertices=simp["vertices"], triangles=simp["triangles"]) if simp else None)
        ref = vol.get("refine")             # ... nor what the edge split added
        split_v, split_t = (sum(r["marked"] for r in ref["rounds"]), sum(r["new_triangles"] for r in ref["rounds"])) if ref else (0, 0)
        if (fil or ref) and not first:
            first = dict(vertices=verts.shape[0] - (fil["filled"] if fil else 0) - split_v,
                         triangles=tris.shape[0] - (fil["new_triangles"] if fil else 0) - split_t)
        print(f"rank {rank}: mesh of {len(pc.keyframes)} keyframes: {vol['nx']} x {vol['ny']} x {vol['nz']} = {vol['voxels']} voxels of {mesh['voxel']:g} m "
              f"(truncation {mesh['trunc']:g} m), {vol['touched']} touched, {first['vertices'] if first else verts.shape[0]} vertices, "
              f"{first['triangles'] if first else tris.shape[0]} triangles -> {path}")
        if flt:
            print(f"rank {rank}: mesh components: {flt['kept_components']} of {flt['components']} kept, {flt['vertices']} -> {flt['kept_vertices']} vertices, "
                  f"{flt['triangles']} -> {flt['kept_triangles']} triangles")
        if simp:
            print(f"rank {rank}: mesh simplify: {simp['clusters']} clusters of {args.mesh_simplify:g} m, triangles {simp['lost']} lost, {simp['collapsed']} collapsed, "
                  f"{simp['duplicate']} duplicate, {simp['kept']} kept, {simp['vertices']} -> {simp['out_vertices']} vertices")
        if fil:
            print(f"rank {rank}: mesh fill holes: {fil['loops']} loops, {fil['filled']} filled, {fil['outlines']} outlines, {fil['too_long']} too long, "
                  f"{fil['blocked']} blocked half-edges, {fil['new_triangles']} new triangles")
        if ref:
            print(f"rank {rank}: mesh refine: edges above {ref['max_edge']:g} m split in {ref['rounds_run']} rounds, "
                  f"{split_v} new vertices, {split_t} new triangles, "
                  f"{ref['left']} edges left above it")
        den = vol.get("denoise")
        if den:
            print(f"rank {rank}: mesh denoise: {den['normal_iterations']} normal iterations with threshold {den['threshold']:g}, "
                  f"{den['vertex_iterations']} vertex iterations, longest row {den['longest_row']}, {den['empty_rows']} vertices without a triangle")
        smo = vol.get("smooth")
        if smo:
            print(f"rank {rank}: mesh smooth: {smo['iterations']} iterations of lambda {smo['lam']:g}, mu {smo['mu']:g}, {smo['edges']} edges, "
                  f"{smo['boundary_vertices']} boundary vertices, {'pinned' if smo['pin_boundary'] else 'not pinned'}")
        aligned = vol.get("colour_align")
        if aligned:
            from rgbid import colouralign as CA
            for line in CA.figure_lines(aligned["figures"], aligned["results"]):
                print(f"rank {rank}: mesh {line}")
        rec = vol.get("recolour")
        if rec:
            print(f"rank {rank}: mesh recolour ({rec['mode']}): {rec['coloured']} of {rec['vertices']} vertices coloured from {len(pc.keyframes)} keyframes; pairs: "
                  + ", ".join(f"{rec[k]} {k}" for k in ("gated", "outside", "hidden", "unmeasured", "averted", "taken")))
        if texture is not None:
            obj = args.mesh_texture
            if world > 1:
                root, ext = os.path.splitext(obj)
                obj = f"{root}.rank{rank}{ext}"
            nrm = fused[3] if args.mesh_normals else None
            try:
                tex = TX.texture_mesh(ctx, verts, tris, aligned["keyframes"] if aligned else pc.keyframes, tuple(args.K), args.rows, args.cols, normals=nrm, colours=cols, **texture)
                TX.write_obj(obj, verts, tris, tex["uv"], tex["atlas"], nrm)
            except ValueError as e:
                sys.exit(f"rank {rank}: --mesh-texture: {e}")
            lay, total = tex["layout"], RC.counts_total(tex["counts"])
            print(f"rank {rank}: mesh texture ({texture['mode']}): {tris.shape[0]} triangles, patch {texture['patch']}, atlas {lay['W']} x {lay['H']}, "
                  f"{tex['textured']} of {tex['texels']} texels textured from {len(pc.keyframes)} keyframes, {tex['fallback']} from the vertex colours; pairs: "
                  + ", ".join(f"{total[k]} {k}" for k in RC.COUNTS) + f" -> {obj}")
        if args.mesh_deviation is not None or args.mesh_reference:
            dev = lambda x: torch.from_numpy(np.ascontiguousarray(x.view(np.int32) if x.dtype == np.uint32 else x)).to(verts.device)
            try:
                if args.mesh_deviation is not None:
                    raw = fused[-1].extract(mesh["min_weight"], colours=False)
                    figures = MD.mesh_deviation(ctx, verts, tris, raw[0], raw[2], args.mesh_deviation)
                    print(f"rank {rank}: mesh deviation: written -> extracted: {MD.summary_line(figures['a_to_b'])}")
                    print(f"rank {rank}: mesh deviation: extracted -> written: {MD.summary_line(figures['b_to_a'])}")
                if reference is not None and args.mesh_reference_register:
                    from rgbid import meshreg as MR
                    reg = MR.register_mesh(ctx, verts, tris, dev(reference[0]), dev(reference[2]), reference_distance)
                    for line in MR.pose_lines(reg):
                        print(f"rank {rank}: mesh reference: {line}")
                    for word, figures in (("before", reg["before"]), ("after", reg["after"])):
                        if figures is not None:
                            print(f"rank {rank}: mesh reference ({word}): written -> {args.mesh_reference}: {MD.summary_line(figures['a_to_b'])}")
                            print(f"rank {rank}: mesh reference ({word}): {args.mesh_reference} -> written: {MD.summary_line(figures['b_to_a'])}")
                elif reference is not None:
                    figures = MD.mesh_deviation(ctx, verts, tris, dev(reference[0]), dev(reference[2]), reference_distance)
                    print(f"rank {rank}: mesh reference: written -> {args.mesh_reference}: {MD.summary_line(figures['a_to_b'])}")
                    print(f"rank {rank}: mesh reference: {args.mesh_reference} -> written: {MD.summary_line(figures['b_to_a'])}")
            except (ValueError, RuntimeError) as e:
                sys.exit(f"rank {rank}: --mesh-deviation / --mesh-reference: {e}")
            finally:
                if keep and not cast:                       # otherwise the ray casts below close the volume
                    fused[-1].close()
        if cast:
            volume = fused[-1]
            try:
                Kt, kfs_all = tuple(args.K), pc.keyframes
                if args.mesh_render_check:
                    figures = TS.surface_agreement(volume, kfs_all, Kt, args.rows, args.cols, args.mesh_render_step, mesh["min_weight"])
                    run = TS.agreement_summary(figures)
                    print(f"rank {rank}: mesh render check: {len(figures)} keyframes, {run['pixels']} pixels, median of medians {run['median']:.6f} m, "
                          f"largest 90 % {run['p90']:.6f} m")
                if args.mesh_render:
                    from rgbid import render as RD
                    os.makedirs(args.mesh_render, exist_ok=True)
                    for a in range(0, len(kfs_all), volume.max_views):
                        kfs = kfs_all[a:a + volume.max_views]
                        views = volume.raycast(np.stack([k["R"] for k in kfs]), np.stack([k["t"] for k in kfs]), Kt, args.rows, args.cols,
                                               args.mesh_render_step, mesh["min_weight"])
                        for j in range(len(kfs)):
                            name = f"view_{a + j:04d}" if world == 1 else f"view_rank{rank}_{a + j:04d}"
                            tum.write_png(os.path.join(args.mesh_render, name + ".png"), views["colour"][j].cpu().numpy())
                            tum.write_png(os.path.join(args.mesh_render, name + "_depth.png"), RD.depth_png(views["depth"][j]))
                            tum.write_png(os.path.join(args.mesh_render, name + "_shaded.png"), TS.shade(views["normal"][j]))
                    print(f"rank {rank}: {len(kfs_all)} ray-cast views of the volume -> {args.mesh_render}")
            finally:
                volume.close()
        if args.mesh_raster or args.mesh_raster_check:
            from rgbid import raster as RS
            from rgbid import render as RD
            Kt, kfs_all = tuple(args.K), pc.keyframes
            try:
                if args.mesh_raster_check:
                    figures = RS.mesh_agreement(ctx, verts, tris, kfs_all, Kt, args.rows, args.cols)
                    for i, f in enumerate(figures):
                        print(f"rank {rank}: mesh raster check: keyframe {i}: {f['pixels']} pixels, median {f['median']:.6f} m, 90 % {f['p90']:.6f} m")
                    run = RD.agreement_summary(figures)
                    print(f"rank {rank}: mesh raster check: {len(figures)} keyframes, {run['pixels']} pixels, median of medians {run['median']:.6f} m, "
                          f"largest 90 % {run['p90']:.6f} m")
                if args.mesh_raster:
                    os.makedirs(args.mesh_raster, exist_ok=True)
                    nrm = fused[3] if args.mesh_normals else None
                    outs = ("depth", "colour", "normal") if args.mesh_normals else ("depth", "colour")
                    rs = RS.Rasteriser(ctx, max(verts.shape[0], 1), max(tris.shape[0], 1), args.rows * args.cols * min(RS.VIEW_CHUNK, len(kfs_all)))
                    try:
                        for a in range(0, len(kfs_all), RS.VIEW_CHUNK):
                            kfs = kfs_all[a:a + RS.VIEW_CHUNK]
                            views = rs.render(verts, tris, np.stack([k["R"] for k in kfs]), np.stack([k["t"] for k in kfs]), Kt, args.rows, args.cols,
                                              cols, nrm, outputs=outs)
                            for j in range(len(kfs)):
                                name = f"mesh_{a + j:04d}" if world == 1 else f"mesh_rank{rank}_{a + j:04d}"
                                tum.write_png(os.path.join(args.mesh_raster, name + ".png"), views["colour"][j].cpu().numpy())
                                tum.write_png(os.path.join(args.mesh_raster, name + "_depth.png"), RD.depth_png(views["depth"][j]))
                                if args.mesh_normals:
                                    tum.write_png(os.path.join(args.mesh_raster, name + "_shaded.png"), TS.shade(views["normal"][j]))
                    finally:
                        rs.close()
                    print(f"rank {rank}: {len(kfs_all)} rasterised views of the mesh -> {args.mesh_raster}")
            except ValueError as e:
                sys.exit(f"rank {rank}: --mesh-raster: {e}")
        if args.mesh_align_check:
            try:
                figures = TS.align_check(ctx, pc.keyframes, tuple(args.K), args.rows, args.cols, points=pc.points, levels=align_levels, **mesh)
            except ValueError as e:
                sys.exit(f"rank {rank}: --mesh-align-check: {e}")
            run = TS.align_check_summary(figures)
            print(f"rank {rank}: mesh align check: {run['views']} keyframes aligned to the model of the others: correction median "
                  f"{run['rotation_median']:.6f} rad {run['translation_median']:.6f} m, largest {run['rotation_max']:.6f} rad {run['translation_max']:.6f} m; "
                  + ", ".join(f"{n} {w}" for w, n in run["status"].items()))
    if comm is not None:
        comm.close()
    if rank == 0:
        tum.write_trajectory(args.out, stamps, R, t)
        print(f"{len(frames)} frames in {args.chunks} chunks on {world} GPU(s): {el:.3f} s ({len(frames) / el:.1f} frames/s incl. engine set-up) -> {args.out}")
    ctx.close()
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
