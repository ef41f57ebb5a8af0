"""Coloured point clouds of exported keyframes (binding of include/rgbid_cloud.h).

The reference turns every keyframe into a point cloud (KeyframeManager::computeAlignedPointCloud, src/keyframe_manager.cpp:438-528):
every pixel whose 1/iD and normal x are not NaN, placed with the keyframe's world pose, with its colour; its viewer draws the "novel"
part, the pixels whose overlap mask is 0.  `Cloud.build` does that on the device for a batch of keyframes in the engine's packed
export layout (Engine.keyframe_sources) and returns 32-byte records in keyframe order, raster order inside a keyframe.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, ci, u64, vp

ALL, NOVEL_ONLY = 0, 1
FLAG_NOVEL = 1
MODES = {"all": ALL, "novel": NOVEL_ONLY}

# rgbid_cloud_point: world position, world normal, pixel index (y * cols + x), colour, flags (bit 0: overlap mask 0)
POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("pixel", "<u4"),
                        ("r", "u1"), ("g", "u1"), ("b", "u1"), ("flags", "u1")])
assert POINT_DTYPE.itemsize == 32

SIGNATURES = {
    "rgbid_cloud_create": (vp, vp, ci, ci, ci),
    "rgbid_cloud_destroy": (vp,),
    "rgbid_cloud_kinv": (vp, vp),
    "rgbid_cloud_plan": (vp, ci, vp, vp, ci, vp),
    "rgbid_cloud_emit": (vp, vp, u64),
}
EXPORTS = list(SIGNATURES)


class Source(C.Structure):
    """rgbid_cloud_src: a packed export block in device memory and the keyframe's world pose R_WC (row-major) | t_WC."""
    _fields_ = [("block_dev", C.c_void_p), ("R", C.c_double * 9), ("t", C.c_double * 3)]


def source(block_dev, R, t):
    R = np.asarray(R, np.float64).reshape(9); t = np.asarray(t, np.float64).reshape(3)
    return Source(C.c_void_p(int(block_dev)), (C.c_double * 9)(*R), (C.c_double * 3)(*t))


def kinv(K):
    """The inverse of K = [fx 0 cx; 0 fy cy; 0 0 1] the library uses (Eigen's cofactor form on the float K widened to double), [3, 3]."""
    k = (C.c_float * 4)(*[float(v) for v in K])
    out = (C.c_double * 9)()
    check(_lib.bind(SIGNATURES).rgbid_cloud_kinv(k, out))
    return np.array(out[:], np.float64).reshape(3, 3)


def records(points):
    """assert that `points` is a contiguous CUDA uint8 tensor [M, 32] of 32-byte records (what the filters over a cloud take); -> points"""
    assert isinstance(points, torch.Tensor) and points.is_cuda and points.dtype == torch.uint8 and points.dim() == 2 and points.shape[1] == 32, \
        "points: a CUDA uint8 tensor [M, 32] of rgbid_cloud_point records"
    assert points.is_contiguous(), "points must be contiguous"
    return points


def records_out(out):
    """assert that `out` can take the 32-byte records of an emit: a contiguous CUDA uint8 tensor [>= M, 32]; -> out"""
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.dim() == 2 and out.shape[1] == 32
    return out


def as_numpy(points):
    """[M, 32] uint8 records (a device or host tensor, or a numpy array) -> structured array of POINT_DTYPE"""
    a = points.cpu().numpy() if isinstance(points, torch.Tensor) else np.asarray(points)
    return np.ascontiguousarray(a).view(POINT_DTYPE).reshape(-1)


class Cloud(_lib.CtxHandle):
    """Point-cloud builder for keyframes of rows x cols pixels, up to max_keyframes per build, on the context's stream."""
    _destroy, _signatures = "rgbid_cloud_destroy", SIGNATURES

    def __init__(self, ctx, rows, cols, max_keyframes):
        super().__init__(ctx)
        self.rows, self.cols, self.max_keyframes = int(rows), int(cols), int(max_keyframes)
        self._created(self.L.rgbid_cloud_create(C.byref(self._h), ctx._h, self.rows, self.cols, self.max_keyframes))

    def plan(self, sources, K, mode="novel"):
        """count pass: -> offsets (uint64 [n + 1]; offsets[n] = number of points).  Synchronises."""
        n = len(sources)
        arr = (Source * max(n, 1))(*sources)
        k = (C.c_float * 4)(*[float(v) for v in K])
        offsets = np.zeros(n + 1, np.uint64)
        check(self.L.rgbid_cloud_plan(self._h, n, arr, k, MODES[mode] if isinstance(mode, str) else int(mode), offsets.ctypes.data_as(C.c_void_p)))
        return offsets

    def emit(self, out):
        """write the points of the last plan into `out` (CUDA uint8 tensor [>= M, 32]).  Asynchronous on the context's stream."""
        records_out(out)
        check(self.L.rgbid_cloud_emit(self._h, self.ptr(out), C.c_ulonglong(out.shape[0])))

    def build(self, sources, K, mode="novel"):
        """-> (points: CUDA uint8 [M, 32] of rgbid_cloud_point records, offsets: uint64 [n + 1]); as_numpy(points) is the structured view.
        The source blocks must stay valid and unchanged until this returns (it synchronises)."""
        offsets = self.plan(sources, K, mode)
        out = torch.empty((int(offsets[-1]), 32), dtype=torch.uint8, device=self._dev)
        self.ctx.wait_torch_stream()   # the output is torch's allocation
        self.emit(out)
        self.ctx.sync()
        return out, offsets


PLY_PROPS = ("x", "y", "z", "nx", "ny", "nz")


def ply_bytes(points):
    """binary little-endian PLY of the records, in record order: x y z nx ny nz (float), red green blue (uchar); 27 B per vertex"""
    p = as_numpy(points)
    head = ("ply\nformat binary_little_endian 1.0\ncomment rgbid keyframe point cloud\n"
            f"element vertex {len(p)}\n"
            + "".join(f"property float {n}\n" for n in PLY_PROPS)
            + "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    v = np.empty(len(p), np.dtype([(n, "<f4") for n in PLY_PROPS] + [("red", "u1"), ("green", "u1"), ("blue", "u1")]))
    for n in PLY_PROPS:
        v[n] = p[n]
    v["red"], v["green"], v["blue"] = p["r"], p["g"], p["b"]
    return head.encode("ascii") + v.tobytes()


def write_ply(path, points):
    with open(path, "wb") as f:
        f.write(ply_bytes(points))


class ChunkCloud:
    """The cloud of a chunked run (sequence.track_chunked): `points` CUDA uint8 [M, 32], `offsets` uint64 [n + 1] (keyframe i's records are
    points[offsets[i]:offsets[i + 1]]) and per keyframe its chunk, export number, global frame and world pose (`keyframes`)."""

    def __init__(self, points, offsets, keyframes):
        self.points, self.offsets, self.keyframes = points, offsets, keyframes

    def __len__(self):
        return int(self.offsets[-1])

    def numpy(self):
        return as_numpy(self.points)


def chunk_cloud(ctx, eng, lanes, R, t, K, mode, steps, depthinv=False, colour=False):
    """points of every keyframe the given engine lanes exported: lanes = [(lane, chunk, first global frame of the chunk)]; R, t = the
    composed trajectory.  A keyframe's world pose is the trajectory's pose at its global frame (first frame + header id).
    depthinv: also keep each export's inverse-depth plane, a CUDA float32 [rows, cols] copy, as the keyframe's `depthinv` (what
    rgbid.render.depth_agreement compares a rendering with).
    colour: also keep each export's colour area, a CUDA uint8 [rows, cols, 3] copy, as the keyframe's `colour` (what rgbid.tsdf.fuse
    colours a mesh with)."""
    counts = eng.keyframe_counts()
    pairs = [(lane, s) for lane, _, _ in lanes for s in range(int(counts[lane]))]
    for lane, _, _ in lanes:
        assert counts[lane] <= steps, (lane, counts[lane], steps)   # at most one export per step (engine.hip reset_integration_keyframe)
    srcs, hdrs = eng.keyframe_sources(pairs)
    first = {lane: (chunk, f0) for lane, chunk, f0 in lanes}
    keyframes = []
    for i, h in enumerate(hdrs):
        chunk, f0 = first[h["lane"]]
        f = f0 + h["id"]
        srcs[i] = source(srcs[i].block_dev, R[f], t[f])
        keyframes.append(dict(chunk=chunk, seq=h["seq"], frame=f, R=np.asarray(R[f]), t=np.asarray(t[f]), header_R=h["R"], header_t=h["t"]))
    if not srcs:
        return ChunkCloud(torch.empty((0, 32), dtype=torch.uint8, device=f"cuda:{ctx.device}"), np.zeros(1, np.uint64), keyframes)
    cl = Cloud(ctx, eng.cfg.rows, eng.cfg.cols, len(srcs))
    try:
        pts, off = cl.build(srcs, K, mode)
    finally:
        cl.close()
    if depthinv:
        N = eng.cfg.rows * eng.cfg.cols
        for kf, src in zip(keyframes, srcs):               # the block: mask u8[N] | colours u8[3N] | inverse depth f32[N] | normals
            kf["depthinv"] = torch.empty((eng.cfg.rows, eng.cfg.cols), dtype=torch.float32, device=f"cuda:{ctx.device}")
        ctx.wait_torch_stream()
        for kf, src in zip(keyframes, srcs):
            check(ctx.L.rgbid_memcpy_d2d(ctx._h, C.c_void_p(kf["depthinv"].data_ptr()), C.c_void_p(src.block_dev + 4 * N), C.c_size_t(4 * N)))
        ctx.sync()
    if colour:
        N = eng.cfg.rows * eng.cfg.cols
        for kf in keyframes:
            kf["colour"] = torch.empty((eng.cfg.rows, eng.cfg.cols, 3), dtype=torch.uint8, device=f"cuda:{ctx.device}")
        ctx.wait_torch_stream()
        for kf, src in zip(keyframes, srcs):
            check(ctx.L.rgbid_memcpy_d2d(ctx._h, C.c_void_p(kf["colour"].data_ptr()), C.c_void_p(src.block_dev + N), C.c_size_t(3 * N)))
        ctx.sync()
    return ChunkCloud(pts, off, keyframes)
