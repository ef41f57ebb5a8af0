"""Tracking a recorded sequence with the batched engine: every lane of the engine tracks one contiguous chunk
(rgbid.dist.chunk_ranges), all chunks advance in lock-step, and the per-frame records of all chunks are composed into one
trajectory.  With torch.distributed initialised, each rank takes its block of chunks (rgbid.dist.rank_chunks) and the
392-byte records {frame id, status, frame-to-frame R | t, covariance} are all-gathered -- the only collective on the path --
through the C-ABI helper over RCCL (rgbid_dist_gather_records) when `comm` is given, else through torch.distributed."""
import numpy as np
import torch

from . import dist as D
from . import engine as E


def track_chunked(ctx, depth, rgb, n_chunks, K, group=None, comm=None, cloud=None, optimise=None, loops=None, loop_options=None, segment=None,
                  keyframe_depth=False, keyframe_colour=False, **cfg_kw):
    """depth [T, rows, cols] 16-bit, rgb [T, rows, cols, 3] uint8 CUDA tensors of ONE sequence.
    Returns (R [T,3,3], t [T,3], ranges); the per-frame status / covariance are in track_chunked.last = (status, cov).

    cloud = "novel" or "all" also builds the coloured point cloud of every keyframe the rank's chunks exported (rgbid.cloud; the novel
    cloud is what the reference's viewer draws) and returns it as a fourth value, a rgbid.cloud.ChunkCloud.  The engine then keeps an
    export ring of keyframe_capacity = chunk length slots per lane -- a lane exports at most one keyframe per step, so no export is
    overwritten -- which costs 20 * rows * cols * chunk length bytes of device memory per lane (an allocation failure is raised).
    Each keyframe is placed with the composed trajectory's pose of the frame it was created at, so the cloud lines up with the
    trajectory; the final, never-exported keyframe of each chunk has no points.

    optimise = "auto" | "multilevel" | "single" runs the pose-graph back-end once over the whole run (rgbid.posegraph.optimise_run, the
    reference's final performOptimisation, keyframe_manager.cpp:229-243): SEQ_ODO from the records, SEQ_KF from the export headers, and with
    loops = "auto", "appearance" or [(kf_a, kf_b), ...] (export indices in frame order) LC_KF constraints from the dense verifier; "auto"
    proposes candidates by distance on the trajectory, "appearance" by features, Hamming matching and RANSAC without any pose
    (rgbid.loopfeat).  optimise="auto" uses multilevel
    when every keyframe-level component is anchored, else single level (a chunk's keyframe chain ends at its last export, so chunked runs
    without seam-crossing loops run single level).  The returned trajectory (and the cloud) are then the optimised ones; what ran is in
    track_chunked.last_optimise (mode, status, chi2, loops).  It needs the whole run on one rank.  loop_options: keyword arguments of
    rgbid.posegraph.loop_constraints (radius, angle, gate, min_separation) and, with loops = "appearance", of rgbid.loopfeat.appearance_loops
    (max_keypoints, score_threshold, per_query, and levels / scale of the feature pyramid: one level by default, the reference runs 8 at 1.2).

    keyframe_depth = True (with cloud) keeps every exported keyframe's inverse-depth plane on the device as `depthinv` of the cloud's
    keyframes, for rgbid.render.depth_agreement; with optimise the cloud placed with the trajectory BEFORE the optimisation is left in
    track_chunked.last_cloud_before as well, so that the agreement can be compared across it.

    keyframe_colour = True (with cloud) keeps every exported keyframe's colours on the device as `colour` of the cloud's keyframes (uint8
    [rows, cols, 3]), for rgbid.tsdf.fuse."""
    if cloud not in (None, "novel", "all"):
        raise ValueError(f"cloud must be None, 'novel' or 'all', not {cloud!r}")
    if optimise not in (None, "auto", "multilevel", "single"):
        raise ValueError(f"optimise must be None, 'auto', 'multilevel' or 'single', not {optimise!r}")
    if loops is not None and optimise is None:
        raise ValueError("loops needs optimise")
    T, rows, cols = depth.shape
    ranges = D.chunk_ranges(T, n_chunks)
    distributed = torch.distributed.is_available() and torch.distributed.is_initialized()
    world = torch.distributed.get_world_size(group) if distributed else 1
    rank = torch.distributed.get_rank(group) if distributed else 0
    mine = D.rank_chunks(n_chunks, world, rank)
    lanes = D.lanes_per_rank(n_chunks, world)          # ranks owning one chunk fewer pad with a lane that re-tracks their last chunk (never read)
    owned = mine + [mine[-1] if mine else 0] * (lanes - len(mine))
    L = max(b - a + 1 for a, b in ranges)
    if optimise is not None and world > 1:
        raise ValueError("optimise needs the whole run on one rank (torch.distributed has several)")
    if cloud is not None or optimise is not None or segment is not None:
        cfg_kw = dict(cfg_kw, keyframe_capacity=L)
    eng = E.Engine(ctx, E.default_config(rows=rows, cols=cols, lanes=lanes, K=K, record_capacity=L, **cfg_kw))
    # Lane-major staging of the whole run, built once and kept alive until the records are read: the engine consumes its inputs
    # asynchronously on its own HIP stream, so per-step temporaries (torch would recycle them on ITS stream) must not be used.
    idx = torch.tensor([[min(ranges[c][0] + j, ranges[c][1]) for c in owned] for j in range(L)], device=depth.device)  # [L, lanes]
    depth_l = depth[idx.reshape(-1)].reshape(L, lanes, rows, cols).contiguous()   # shorter chunks repeat their last frame (unused)
    rgb_l = rgb[idx.reshape(-1)].reshape(L, lanes, rows, cols, 3).contiguous()
    torch.cuda.synchronize(depth.device)
    for j in range(L):
        eng.step(depth_l[j], rgb_l[j])
    packed = D.pack_engine_records(eng, 0, L)         # device: [lanes][L] records
    if comm is not None:
        allb = comm.gather(packed, lanes * L)
        ctx.sync()
        allrec = allb.cpu().numpy().view(D.GATHER_DTYPE).reshape(world, lanes, L)
    else:
        ctx.sync()
        local = packed.cpu().numpy().view(D.GATHER_DTYPE).reshape(lanes, L)
        allrec = D.gather_records_torch(local, group) if distributed else local[None]
    R, t, st, cov = D.compose_trajectory(allrec, world, n_chunks, ranges)
    track_chunked.last = (st, cov)
    R0, t0 = R, t
    if optimise is not None:
        try:
            R, t = _optimise(ctx, eng, mine, ranges, allrec[0], R, t, K, optimise, loops, loop_options or {}, L)
        except Exception:
            eng.close()
            raise
    if segment is not None:
        try:
            track_chunked.last_labels = _segment(ctx, eng, mine, K, segment)
        except Exception:
            eng.close()
            raise
    if cloud is None:
        eng.close()
        return R, t, ranges
    from . import cloud as CL
    try:
        lanes_of = [(i, c, ranges[c][0]) for i, c in enumerate(mine)]
        pc = CL.chunk_cloud(ctx, eng, lanes_of, R, t, K, cloud, steps=L, depthinv=keyframe_depth, colour=keyframe_colour)
        if keyframe_depth and optimise is not None:
            before = CL.chunk_cloud(ctx, eng, lanes_of, R0, t0, K, cloud, steps=L)
            for kf, after in zip(before.keyframes, pc.keyframes):
                kf["depthinv"] = after["depthinv"]
            track_chunked.last_cloud_before = before
    finally:
        eng.close()
    return R, t, ranges, pc


def _segment(ctx, eng, mine, K, options, batch=16):
    """segment=dict(k=, min_size=, max_segments=) of track_chunked: the superjut labels of every keyframe this rank's lanes exported
    (rgbid.segment, on the ring's blocks) -> [(chunk, export number, labels int32 [rows, cols])], left in track_chunked.last_labels"""
    from . import segment as SG
    counts = eng.keyframe_counts()
    pairs = [(lane, s) for lane in range(len(mine)) for s in range(int(counts[lane]))]
    if not pairs:
        return []
    srcs, _ = eng.keyframe_sources(pairs)
    labels = SG.segment_batches(ctx, srcs, K, eng.cfg.rows, eng.cfg.cols, batch, options.get("max_segments"),
                                lambda sg, s, res: res[0].cpu().numpy(), k=options.get("k"), min_size=options.get("min_size"))
    labels = [l for part in labels for l in part]
    return [(mine[lane], seq, labels[i]) for i, (lane, seq) in enumerate(pairs)]


def _optimise(ctx, eng, mine, ranges, rec, R, t, K, optimise, loops, loop_options, steps):
    """the pose-graph pass of track_chunked: records and exports of the lanes of this (single) rank -> optimised R, t"""
    from . import posegraph as PG
    counts = eng.keyframe_counts()
    chunk_records, first, headers, keyframes = [], [], [], []
    for lane, c in enumerate(mine):
        a, b = ranges[c]
        chunk_records.append(rec[lane, :b - a + 1])
        first.append(a)
        assert counts[lane] <= steps, (lane, counts[lane], steps)   # at most one export per step: the ring holds them all
        for s in range(int(counts[lane])):
            h = eng.read_keyframe(lane, s, images=loops is not None)
            headers.append((lane, h))
            if loops is not None:
                keyframes.append(dict(frame=a + int(h["id"]), depthinv=h["depthinv"], colors=h["colors"]))
    order = sorted(range(len(keyframes)), key=lambda i: keyframes[i]["frame"])
    if loops == "appearance" and loop_options.get("mask_level") and "blocks" not in loop_options and keyframes:
        srcs, _ = eng.keyframe_sources([(lane, int(h["seq"])) for lane, h in headers])    # the masks read the ring's blocks on the device
        loop_options = dict(loop_options, blocks=[srcs[i] for i in order])
    keyframes = [keyframes[i] for i in order]
    Ro, to, info = PG.optimise_run(ctx, R, t, chunk_records, first, headers, keyframes, K, optimise, loops, **loop_options)
    track_chunked.last_optimise = info
    return Ro, to

