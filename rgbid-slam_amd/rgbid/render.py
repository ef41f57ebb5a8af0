"""The map seen from camera poses, without a window (binding of include/rgbid_render.h).

`Renderer.render` projects the 32-byte records of `rgbid.cloud` (or what `rgbid.outlier` / a caller left of them) into V pinhole
cameras on the device and keeps the nearest record per pixel: its index, depth, colour and camera-frame normal, byte-identical to the
numpy restatement of the contract.  `depth_agreement` renders the map at every keyframe's own pose and compares
what the other keyframes put there with what the keyframe measured: a quality figure of a map that needs no ground truth.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _args as A
from . import _lib
from ._lib import check, ci, f32, u64, vp
from .cloud import records

MAX_SPLAT = 4
MAX_POINTS = (1 << 31) - 1
MAX_DIM = 1 << 20
VIEW_CHUNK = 16
EMPTY = 0xFFFFFFFF
NAN_BITS = 0x7FFFFFFF
DEPTH_PNG_SCALE = 5000.0                # a TUM depth file holds metres * 5000 (millimetres * 5); 0 = no measurement
SIGNATURES = {
    "rgbid_render_create": (vp, vp, u64, u64),
    "rgbid_render_destroy": (vp,),
    "rgbid_render_pose_cw": (vp, vp),
    "rgbid_render_views": (vp, vp, u64, ci, vp, vp, ci, ci, ci, f32, f32, vp, vp, vp, vp),
    "rgbid_render_timing": (vp, ci, vp),
    "rgbid_render_stats": (vp, ci, vp),
}
EXPORTS = list(SIGNATURES)
STAGES = ("clear", "splat", "resolve")
PLANES = ("index", "depth", "colour", "normal")


class Pose(C.Structure):
    """rgbid_render_pose: a camera's world pose R_WC (row-major) | t_WC"""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3)]


def image_size(rows, cols, views=1, max_pixels=None):
    """-> (rows, cols) as the library takes them: 1 .. 2^20 each, and rows * cols * views <= max_pixels when given (ValueError otherwise)"""
    r, c, v = A.integer("rows", rows), A.integer("cols", cols), A.integer("views", views)
    if not (1 <= r <= MAX_DIM and 1 <= c <= MAX_DIM):
        raise ValueError(f"rows and cols must lie in [1, 2^20], got {rows!r} x {cols!r}")
    if v < 1:
        raise ValueError(f"at least one view, got {views!r}")
    if max_pixels is not None and r * c * v > max_pixels:
        raise ValueError(f"{v} views of {r} x {c} pixels are more than the renderer's {max_pixels} pixels")
    return r, c


def splat_arg(splat):
    """-> the splat half-width: an integer in 0 .. 4 (ValueError otherwise)"""
    return A.integer_in("splat", splat, 0, MAX_SPLAT, f"[0, {MAX_SPLAT}]")


def depth_range(z_min, z_max):
    """-> (z_min, z_max) as the float32 values the library receives: finite, 0 < z_min <= z_max (ValueError otherwise)"""
    lo, hi = (A.float32(z, f"z_min, z_max: numbers, got {z_min!r}, {z_max!r}", over="warn") for z in (z_min, z_max))
    if not (math.isfinite(lo) and math.isfinite(hi) and 0 < lo <= hi):
        raise ValueError(f"z_min, z_max must be finite with 0 < z_min <= z_max, got {z_min!r}, {z_max!r}")
    return lo, hi


def intrinsics(K):
    """-> K = fx, fy, cx, cy as four finite float32 values, fx and fy not 0 (ValueError otherwise)"""
    try:
        k = np.asarray(K, np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"K: fx, fy, cx, cy, got {K!r}")
    with np.errstate(over="ignore"):
        k32 = k.astype(np.float32)
    if k.shape != (4,) or not np.isfinite(k32).all() or k32[0] == 0 or k32[1] == 0:
        raise ValueError(f"K: four finite numbers fx, fy, cx, cy with fx, fy != 0, got {K!r}")
    return [float(v) for v in k32]


def poses(R, t):
    """world poses R_WC [V, 3, 3] (or [3, 3]) and t_WC [V, 3] (or [3]) -> (R float64 [V, 3, 3], t float64 [V, 3]): V >= 1, every entry
    finite and within float32's range (ValueError otherwise)"""
    try:
        R = np.asarray(R, np.float64); t = np.asarray(t, np.float64)
        R = R.reshape(-1, 3, 3); t = t.reshape(-1, 3)
    except (TypeError, ValueError):
        raise ValueError("R: [V, 3, 3] and t: [V, 3] numbers")
    if len(R) < 1 or len(R) != len(t):
        raise ValueError(f"R and t must hold the same number (>= 1) of views, got {len(R)} and {len(t)}")
    with np.errstate(over="ignore", invalid="ignore"):
        tcw = -np.einsum("vji,vj->vi", R, t)
        ok = np.isfinite(R.astype(np.float32)).all() and np.isfinite(t).all() and np.isfinite(tcw.astype(np.float32)).all()
    if not ok:
        raise ValueError("poses must be finite")
    return np.ascontiguousarray(R), np.ascontiguousarray(t)


def outputs_arg(outputs):
    """-> the requested planes as a tuple out of index, depth, colour, normal (ValueError otherwise)"""
    outs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    if not outs or any(o not in PLANES for o in outs):
        raise ValueError(f"outputs: some of {PLANES}, got {outputs!r}")
    return outs


def pose_cw(R, t):
    """the twelve float32 values r00 .. r22, tx, ty, tz of R_CW | t_CW as the library forms them from one world pose"""
    p = Pose((C.c_double * 9)(*np.asarray(R, np.float64).reshape(9)), (C.c_double * 3)(*np.asarray(t, np.float64).reshape(3)))
    out = (C.c_float * 12)()
    check(_lib.bind(SIGNATURES).rgbid_render_pose_cw(C.byref(p), out))
    return np.array(out[:], np.float32)


class Renderer(_lib.CtxHandle):
    """Renderer for up to max_points records and rows * cols * views <= max_pixels per call, on the context's stream."""
    _destroy, _signatures, _timing, _stages = "rgbid_render_destroy", SIGNATURES, "rgbid_render_timing", STAGES

    def __init__(self, ctx, max_points, max_pixels):
        super().__init__(ctx)
        self.max_points, self.max_pixels = int(max_points), int(max_pixels)
        self._created(self.L.rgbid_render_create(C.byref(self._h), ctx._h, C.c_ulonglong(self.max_points), C.c_ulonglong(self.max_pixels)))

    def render_into(self, points, R, t, K, rows, cols, splat, z_min, z_max, index=None, depth=None, colour=None, normal=None):
        """the raw call: checked arguments, the given CUDA planes (or None) filled asynchronously on the context's stream"""
        records(points)
        R, t = poses(R, t)
        V = len(R)
        rows, cols = image_size(rows, cols, V, self.max_pixels)
        s = splat_arg(splat)
        lo, hi = depth_range(z_min, z_max)
        k = (C.c_float * 4)(*intrinsics(K))
        if points.shape[0] > self.max_points:
            raise ValueError(f"{points.shape[0]} records are more than the renderer's {self.max_points}")
        arr = (Pose * V)(*[Pose((C.c_double * 9)(*R[v].reshape(9)), (C.c_double * 3)(*t[v])) for v in range(V)])
        ptr = self.opt_ptr
        check(self.L.rgbid_render_views(self._h, ptr(points), C.c_ulonglong(points.shape[0]), V, arr, k,
                                        rows, cols, s, C.c_float(lo), C.c_float(hi), ptr(index), ptr(depth), ptr(colour), ptr(normal)))

    def render(self, points, R, t, K, rows, cols, splat=1, z_min=0.05, z_max=20.0, outputs=("depth", "colour")):
        """`points` (CUDA uint8 [M, 32] records) seen from the world poses R [V, 3, 3], t [V, 3] through K = fx, fy, cx, cy -> a dict of the
        requested planes as CUDA tensors with a leading view axis: index int32 [V, rows, cols] (-1 = rgbid.render.EMPTY as two's
        complement: nobody wrote the pixel), depth float32 [V, rows, cols], colour uint8 [V, rows, cols, 3], normal float32
        [V, 3, rows, cols].  Synchronises."""
        outs = outputs_arg(outputs)
        V = len(poses(R, t)[0])
        rows, cols = image_size(rows, cols, V, self.max_pixels)
        shape = {"index": ((V, rows, cols), torch.int32), "depth": ((V, rows, cols), torch.float32),
                 "colour": ((V, rows, cols, 3), torch.uint8), "normal": ((V, 3, rows, cols), torch.float32)}
        planes = {o: torch.empty(shape[o][0], dtype=shape[o][1], device=self._dev) for o in outs}
        self.ctx.wait_torch_stream()   # the records were written, and the planes allocated, on torch's stream
        self.render_into(points, R, t, K, rows, cols, splat, z_min, z_max, **planes)
        self.ctx.sync()
        return planes

    def stats(self, enable=True):
        """count in the following calls; -> the last one's {pairs, writes, atomics}: visible (record, view) pairs, the pixel writes they
        attempted, those that reached the atomic minimum"""
        st = (C.c_ulonglong * 3)()
        check(self.L.rgbid_render_stats(self._h, int(enable), st))
        return dict(zip(("pairs", "writes", "atomics"), (int(v) for v in st)))


def render_views(ctx, points, R, t, K, rows, cols, splat=1, z_min=0.05, z_max=20.0, outputs=("depth", "colour")):
    """one-shot Renderer(ctx, len(points), rows * cols * views).render(...)"""
    outputs_arg(outputs); splat_arg(splat); depth_range(z_min, z_max); intrinsics(K)
    V = len(poses(R, t)[0])
    rows, cols = image_size(rows, cols, V)
    rd = Renderer(ctx, max(points.shape[0], 1), rows * cols * V)
    try:
        return rd.render(points, R, t, K, rows, cols, splat, z_min, z_max, outputs)
    finally:
        rd.close()


def rank_value(sorted_values, q10):
    """the nearest-rank quantile q10 / 10 of ascending values: the element at ceil(q10 n / 10) - 1; NaN of none"""
    n = len(sorted_values)
    return float(sorted_values[(q10 * n + 9) // 10 - 1]) if n else float("nan")


def agreement_of(index, depth, own_depthinv, first, last):
    """one keyframe's figures from a rendering at its pose: index (int32, -1 empty) and depth planes [rows, cols] (torch), the keyframe's
    own inverse depth (numpy float32 [rows, cols]) and its own records' range [first, last) -> dict(pixels, median, p90): the pixels
    where a record of ANOTHER keyframe won and the keyframe measured a depth (iD finite and > 0, z = 1 / iD in float32), and the
    median and 90th percentile (nearest rank) of |z_render - z_keyframe| over them"""
    iD = np.asarray(own_depthinv, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        own = np.where(np.isfinite(iD) & (iD > 0), np.float32(1) / iD, np.float32(np.nan)).astype(np.float32)
    own = torch.from_numpy(own).to(depth.device)
    idx = index.to(torch.int64) & 0xFFFFFFFF
    both = (idx != EMPTY) & ((idx < int(first)) | (idx >= int(last))) & torch.isfinite(own)
    d = torch.sort((depth[both] - own[both]).abs()).values.cpu().numpy()
    return dict(pixels=int(len(d)), median=rank_value(d, 5), p90=rank_value(d, 9))


def depth_agreement(ctx, points, offsets, keyframes, K, rows, cols, splat=1, z_min=0.05, z_max=20.0, batch=VIEW_CHUNK):
    """How well the map agrees with what each keyframe measured.  points, offsets: the records and the per-keyframe offsets of
    rgbid_cloud_plan (keyframe i owns points[offsets[i]:offsets[i + 1]]); keyframes: per keyframe a dict with its world pose R, t and
    its export's inverse depth `depthinv` [rows, cols].  The cloud is rendered at every keyframe's pose; pixels whose winner is one of
    the keyframe's own records are ignored.  -> per keyframe dict(pixels, median, p90), see agreement_of."""
    assert len(offsets) == len(keyframes) + 1
    out = []
    if not keyframes:
        return out
    rows, cols = image_size(rows, cols)
    batch = max(1, min(int(batch), len(keyframes)))
    rd = Renderer(ctx, max(points.shape[0], 1), rows * cols * batch)
    try:
        for a in range(0, len(keyframes), batch):
            kfs = keyframes[a:a + batch]
            pl = rd.render(points, np.stack([np.asarray(k["R"]) for k in kfs]), np.stack([np.asarray(k["t"]) for k in kfs]), K, rows, cols,
                           splat, z_min, z_max, outputs=("index", "depth"))
            for j, k in enumerate(kfs):
                iD = k["depthinv"]
                iD = iD.cpu().numpy() if isinstance(iD, torch.Tensor) else iD
                out.append(agreement_of(pl["index"][j], pl["depth"][j], iD, offsets[a + j], offsets[a + j + 1]))
    finally:
        rd.close()
    return out


def agreement_summary(figures):
    """per-keyframe figures -> the run's: dict(pixels = their sum, median = the median of the keyframes' medians, p90 = the largest 90th
    percentile), over the keyframes that have any pixel"""
    have = [f for f in figures if f["pixels"]]
    if not have:
        return dict(pixels=0, median=float("nan"), p90=float("nan"))
    return dict(pixels=sum(f["pixels"] for f in have), median=float(np.median([f["median"] for f in have])), p90=max(f["p90"] for f in have))


def depth_png(depth):
    """a depth plane in metres (NaN = empty) -> uint16 as a TUM depth file holds it: metres * 5000 rounded, empty = 0, clipped at 65535"""
    d = np.asarray(depth.cpu() if isinstance(depth, torch.Tensor) else depth, np.float32)
    with np.errstate(invalid="ignore"):
        v = np.rint(np.where(np.isfinite(d), d, 0).astype(np.float64) * DEPTH_PNG_SCALE)
    return np.clip(v, 0, 65535).astype(np.uint16)
