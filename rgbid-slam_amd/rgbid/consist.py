"""Multi-view consistency filter over keyframe point clouds (binding of include/rgbid_consist.h).

A record goes when other keyframes, looking along their own rays, measured a surface clearly behind it: they saw through the place where
the record claims to be.  `ConsistencyFilter.filter` counts, per record, the keyframes that support it and those that contradict it on the
device, over the 32-byte records of `rgbid.cloud`, the keyframes' poses and their inverse-depth planes as
`sequence.track_chunked(cloud=..., keyframe_depth=True)` leaves them, and returns the kept records unchanged, in input order, byte-identical
to the numpy restatement of the contract.  It comes first in the map chain: `rgbid.outlier`, `rgbid.voxel`,
`rgbid.render` and `rgbid.cloud.write_ply` take its output as they take the unfiltered cloud.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _args as A
from . import _lib
from ._lib import check, ci, u64, vp
from .cloud import records, records_out
from .render import Pose, depth_range, image_size, intrinsics, poses

MAX_POINTS = (1 << 31) - 1
MAX_VIEWS = 65535
MAX_WINDOW = 2
MAX_DIM = 1 << 20
VIEW_CHUNK = 16                         # RGBID_CONSIST_VIEW_CHUNK: more views than this are counted in chunks of it
SIGNATURES = {
    "rgbid_consist_create": (vp, vp, u64, ci),
    "rgbid_consist_destroy": (vp,),
    "rgbid_consist_plan": (vp, vp, u64, ci, vp, vp, vp, ci, ci, vp, vp, vp),
    "rgbid_consist_counts": (vp, vp),
    "rgbid_consist_emit": (vp, vp, u64),
    "rgbid_consist_timing": (vp, ci, vp),
}
EXPORTS = list(SIGNATURES)
STAGES = ("count", "scan", "emit")


class View(C.Structure):
    """rgbid_consist_view: a keyframe's world pose and its inverse-depth plane on the device"""
    _fields_ = [("pose", Pose), ("depthinv_dev", C.c_void_p)]


class Params(C.Structure):
    """rgbid_consist_params"""
    _fields_ = [("tol_rel", C.c_float), ("tol_abs", C.c_float), ("window", C.c_int), ("z_min", C.c_float), ("z_max", C.c_float),
                ("min_support", C.c_uint), ("max_conflicts", C.c_uint)]


def tolerances(tol_rel, tol_abs=0.0):
    """-> (tol_rel, tol_abs) as the float32 values the library receives: finite and >= 0 (ValueError otherwise)"""
    r, a = (A.float32(x, f"tol_rel, tol_abs: numbers, got {tol_rel!r}, {tol_abs!r}") for x in (tol_rel, tol_abs))
    if not (math.isfinite(r) and math.isfinite(a) and r >= 0 and a >= 0):
        raise ValueError(f"tol_rel, tol_abs must be finite and >= 0, got {tol_rel!r}, {tol_abs!r}")
    return r, a


def window_arg(window):
    """-> the window half-width: an integer in 0 .. 2 (ValueError otherwise)"""
    return A.integer_in("window", window, 0, MAX_WINDOW, f"[0, {MAX_WINDOW}]")


def vote_args(min_support, max_conflicts):
    """-> (min_support, max_conflicts): integers in 0 .. 65 535 each (ValueError otherwise)"""
    s, c = A.integer("min_support", min_support), A.integer("max_conflicts", max_conflicts)
    if not (0 <= s <= MAX_VIEWS and 0 <= c <= MAX_VIEWS):
        raise ValueError(f"min_support and max_conflicts must lie in [0, {MAX_VIEWS}], got {min_support!r}, {max_conflicts!r}")
    return s, c


def offsets_arg(offsets, views, n):
    """-> the per-view owner offsets as uint64 [views + 1], or None for None: ascending from 0 to n (ValueError otherwise)"""
    if offsets is None:
        return None
    try:
        o = np.asarray(offsets)
        bad = o.dtype.kind not in "iu" or o.shape != (views + 1,)
    except (TypeError, ValueError):
        bad = True
    if bad:
        raise ValueError(f"offsets: {views + 1} integers, got {offsets!r}")
    o = o.astype(np.int64) if o.dtype.kind == "i" else o
    if o[0] != 0 or o[-1] != n or (o[1:] < o[:-1]).any():
        raise ValueError(f"offsets must ascend from 0 to the number of records ({n}), got {offsets!r}")
    return np.ascontiguousarray(o.astype(np.uint64))


def planes_arg(planes, views, rows, cols, device=None):
    """-> the inverse-depth planes as a list of `views` contiguous CUDA float32 tensors [rows, cols] (ValueError otherwise).  planes: a
    sequence of such tensors (the keyframes' `depthinv`) or one tensor [views, rows, cols]"""
    if isinstance(planes, torch.Tensor):
        planes = list(planes) if planes.dim() == 3 else [planes]
    try:
        planes = list(planes)
    except TypeError:
        raise ValueError("planes: a sequence of CUDA float32 tensors [rows, cols]")
    if len(planes) != views:
        raise ValueError(f"{views} views need {views} planes, got {len(planes)}")
    for p in planes:
        A.cuda_tensor("planes", p, torch.float32, (rows, cols), f"planes: contiguous CUDA float32 tensors [{rows}, {cols}]", device)
    return planes


def offsets_of_kept(counts, offsets, min_support=0, max_conflicts=0, finite=None):
    """the kept records' per-view offsets from the packed counts (int32 / uint32 [n], host or device), the input offsets and the keep rule;
    finite: bool [n], which records took part (None: all of them)"""
    c = (counts.cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)).view(np.uint32)
    keep = ((c & 0xFFFF) >= min_support) & ((c >> 16) <= max_conflicts)
    if finite is not None:
        keep &= np.asarray(finite, bool)
    cum = np.concatenate([[0], np.cumsum(keep, dtype=np.uint64)]).astype(np.uint64)
    return cum[np.asarray(offsets, np.int64)]


class Plan:
    """what rgbid_consist_plan reports: kept (records the emit writes), n, the records that took part, the (record, view) pairs past the
    gates, the records with at least one contradicting view"""

    def __init__(self, kept, n, views, stats):
        self.kept, self.n, self.views = int(kept), int(n), int(views)
        self.finite, self.pairs, self.contradicted = int(stats[0]), int(stats[1]), int(stats[2])

    def __repr__(self):
        return (f"Plan(kept={self.kept}, n={self.n}, views={self.views}, finite={self.finite}, pairs={self.pairs}, "
                f"contradicted={self.contradicted})")


class ConsistencyFilter(_lib.CtxHandle):
    """Consistency filter for up to max_points records and max_views views per plan, on the context's stream."""
    _destroy, _signatures, _timing, _stages = "rgbid_consist_destroy", SIGNATURES, "rgbid_consist_timing", STAGES

    def __init__(self, ctx, max_points, max_views):
        super().__init__(ctx)
        self.max_points, self.max_views = int(max_points), int(max_views)
        self._created(self.L.rgbid_consist_create(C.byref(self._h), ctx._h, C.c_ulonglong(self.max_points), self.max_views))

    def plan(self, points, offsets, planes, R, t, K, rows, cols, tol_rel=0.02, tol_abs=0.0, window=1, min_support=0, max_conflicts=0,
             z_min=0.05, z_max=20.0):
        """count and mark pass over `points` (CUDA uint8 [M, 32] records) against the views R [V, 3, 3], t [V, 3] with the inverse-depth
        `planes` -> Plan.  Synchronises (on the context's stream: records and planes written on torch's stream are waited for first)."""
        records(points)
        R, t = poses(R, t)
        V, n = len(R), points.shape[0]
        rows, cols = image_size(rows, cols)
        if V > self.max_views:
            raise ValueError(f"{V} views are more than the filter's {self.max_views}")
        if n > self.max_points:
            raise ValueError(f"{n} records are more than the filter's {self.max_points}")
        planes = planes_arg(planes, V, rows, cols, self.ctx.device)
        off = offsets_arg(offsets, V, n)
        tr, ta = tolerances(tol_rel, tol_abs)
        lo, hi = depth_range(z_min, z_max)
        s, c = vote_args(min_support, max_conflicts)
        prm = Params(tr, ta, window_arg(window), lo, hi, s, c)
        k = (C.c_float * 4)(*intrinsics(K))
        views = (View * V)(*[View(Pose((C.c_double * 9)(*R[v].reshape(9)), (C.c_double * 3)(*t[v])), planes[v].data_ptr()) for v in range(V)])
        stats = np.zeros(4, np.uint64); kept = C.c_ulonglong()
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_consist_plan(self._h, self.ptr(points), C.c_ulonglong(n), V, views,
                                        off.ctypes.data_as(C.c_void_p) if off is not None else None, k, rows, cols, C.byref(prm),
                                        stats.ctypes.data_as(C.c_void_p), C.byref(kept)))
        return Plan(kept.value, n, V, stats)

    def counts(self, out):
        """write support | conflicts << 16 of the last plan's records, in input order, into `out` (CUDA int32 / uint32 tensor [>= n]).
        Asynchronous on the context's stream."""
        assert out.is_cuda and out.element_size() == 4 and not out.is_floating_point() and out.is_contiguous() and out.dim() == 1
        check(self.L.rgbid_consist_counts(self._h, self.ptr(out)))

    def emit(self, out):
        """write the kept records of the last plan into `out` (CUDA uint8 tensor [>= kept, 32]).  Asynchronous on the context's stream."""
        records_out(out)
        check(self.L.rgbid_consist_emit(self._h, self.ptr(out), C.c_ulonglong(out.shape[0])))

    def filter(self, points, offsets, planes, R, t, K, rows, cols, tol_rel=0.02, tol_abs=0.0, window=1, min_support=0, max_conflicts=0,
               z_min=0.05, z_max=20.0, return_counts=False, return_offsets=False, return_plan=False):
        """-> CUDA uint8 [kept, 32]: the records that at least min_support views support and at most max_conflicts views contradict,
        unchanged, in input order; with return_counts also the int32 [M] counts (support | conflicts << 16); with return_offsets also
        the kept records' per-view offsets (uint64 [V + 1], needs offsets), so that render.depth_agreement runs on the filtered cloud;
        with return_plan also the Plan.  The defaults remove only contradicted records: most novel points are seen by one keyframe alone
        and have support 0.  `points` and `planes` must stay unchanged until this returns (it synchronises)."""
        if return_offsets and offsets is None:
            raise ValueError("return_offsets needs offsets")
        p = self.plan(points, offsets, planes, R, t, K, rows, cols, tol_rel, tol_abs, window, min_support, max_conflicts, z_min, z_max)
        out = torch.empty((p.kept, 32), dtype=torch.uint8, device=self._dev)
        cnt = torch.empty((p.n,), dtype=torch.int32, device=self._dev) if return_counts or return_offsets else None
        self.ctx.wait_torch_stream()   # the outputs are torch's allocations
        if cnt is not None:
            self.counts(cnt)
        self.emit(out)
        self.ctx.sync()
        res = (out,)
        if return_counts:
            res += (cnt,)
        if return_offsets:
            fin = torch.isfinite(points.view(torch.float32)[:, :3]).all(1).cpu().numpy() if p.finite != p.n else None
            off = offsets_of_kept(cnt, offsets, *vote_args(min_support, max_conflicts), finite=fin)
            assert int(off[-1]) == p.kept
            res += (off,)
        if return_plan:
            res += (p,)
        return res if len(res) > 1 else out


def consistency_filter(ctx, points, offsets, planes, R, t, K, rows, cols, tol_rel=0.02, tol_abs=0.0, window=1, min_support=0,
                       max_conflicts=0, z_min=0.05, z_max=20.0, return_counts=False, return_offsets=False, return_plan=False):
    """one-shot ConsistencyFilter(ctx, len(points), views).filter(...)"""
    V = len(poses(R, t)[0])
    if V > MAX_VIEWS:
        raise ValueError(f"at most {MAX_VIEWS} views, got {V}")
    tolerances(tol_rel, tol_abs); window_arg(window); vote_args(min_support, max_conflicts); depth_range(z_min, z_max); intrinsics(K)
    image_size(rows, cols); offsets_arg(offsets, V, points.shape[0])
    cf = ConsistencyFilter(ctx, max(points.shape[0], 1), V)
    try:
        return cf.filter(points, offsets, planes, R, t, K, rows, cols, tol_rel, tol_abs, window, min_support, max_conflicts, z_min, z_max,
                         return_counts, return_offsets, return_plan)
    finally:
        cf.close()
