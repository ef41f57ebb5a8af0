"""Radius outlier filter over keyframe point clouds (binding of include/rgbid_outlier.h).

A record stays when at least `min_neighbours` other records lie within `radius` of it: the isolated mixed-depth points along depth
discontinuities go, the surface stays.  `RadiusFilter.filter` does that on the device over the 32-byte records of `rgbid.cloud` and
returns the kept records unchanged, in input order, bitwise reproducible; `rgbid.voxel` and
`rgbid.cloud.write_ply` take them as they take the unfiltered cloud.
"""
import ctypes as C

import numpy as np
import torch

from . import _args as A
from . import _lib
from ._lib import check, ci, cu, f32, u64, vp
from .cloud import records, records_out

MAX_POINTS = 1 << 31
MAX_CELL = 1 << 18                      # RGBID_OUTLIER_MAX_CELL: the largest |floor(p * inv)| the plan accepts
CELL_FACTOR = np.float32(1.0625)        # RGBID_OUTLIER_CELL_FACTOR: cell size / radius
MIN_RADIUS, MAX_RADIUS = 2.0 ** -60, 2.0 ** 60
SIGNATURES = {
    "rgbid_outlier_create": (vp, vp, u64),
    "rgbid_outlier_destroy": (vp,),
    "rgbid_outlier_plan": (vp, vp, u64, f32, cu, cu, vp, vp),
    "rgbid_outlier_counts": (vp, vp),
    "rgbid_outlier_emit": (vp, vp, u64),
    "rgbid_outlier_timing": (vp, ci, vp),
}
EXPORTS = list(SIGNATURES)
STAGES = ("box", "sort", "cells", "count", "emit")


def radius32(radius):
    """-> the radius as the float32 value the library receives: finite, > 0 and in [2^-60, 2^60] (ValueError otherwise)"""
    r = A.positive32("radius", radius, f"radius: a number, got {radius!r}", over="warn")
    return A.in_range("radius", r, MIN_RADIUS, MAX_RADIUS, "[2^-60, 2^60]", radius)


def neighbour_args(min_neighbours, cap=None):
    """-> (min_neighbours, cap) as the library takes them: 0 <= min_neighbours <= cap, 1 <= cap < 2^32; the default cap is
    max(min_neighbours, 1) (ValueError otherwise)"""
    m = A.integer("min_neighbours", min_neighbours)
    c = A.integer_in("cap", max(m, 1) if cap is None else cap, 1, (1 << 32) - 1, "[1, 2^32)")
    return A.in_range("min_neighbours", m, 0, c, f"[0, cap = {c}]", min_neighbours), c


def cell_size(radius):
    """the edge of the search grid's cells for this radius, as the library forms it in float32"""
    return np.float32(radius32(radius)) * CELL_FACTOR


class Plan:
    """what rgbid_outlier_plan reports: kept (records the emit writes), n, finite points, occupied cells"""

    def __init__(self, kept, n, stats):
        self.kept, self.n = int(kept), int(n)
        self.finite, self.cells = int(stats[0]), int(stats[1])

    def __repr__(self):
        return f"Plan(kept={self.kept}, n={self.n}, finite={self.finite}, cells={self.cells})"


class RadiusFilter(_lib.CtxHandle):
    """Radius outlier filter for up to max_points input records per plan, on the context's stream."""
    _destroy, _signatures, _timing, _stages = "rgbid_outlier_destroy", SIGNATURES, "rgbid_outlier_timing", STAGES

    def __init__(self, ctx, max_points):
        super().__init__(ctx)
        self.max_points = int(max_points)
        self._created(self.L.rgbid_outlier_create(C.byref(self._h), ctx._h, C.c_ulonglong(self.max_points)))

    def plan(self, points, radius, min_neighbours, cap=None):
        """grid, sort, count and mark pass over `points` (CUDA uint8 [M, 32] rgbid_cloud_point records) -> Plan.  Synchronises (on the
        context's stream: records written on torch's stream are waited for first)."""
        records(points)
        r = radius32(radius)
        m, c = neighbour_args(min_neighbours, cap)
        stats = np.zeros(3, np.uint64); kept = C.c_ulonglong()
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_outlier_plan(self._h, self.ptr(points), C.c_ulonglong(points.shape[0]), C.c_float(r), C.c_uint(c), C.c_uint(m),
                                        stats.ctypes.data_as(C.c_void_p), C.byref(kept)))
        return Plan(kept.value, points.shape[0], stats)

    def counts(self, out):
        """write the clamped neighbour counts of the last plan, in input order, into `out` (CUDA int32 / uint32 tensor [>= n]).
        Asynchronous on the context's stream."""
        assert out.is_cuda and out.element_size() == 4 and not out.is_floating_point() and out.is_contiguous() and out.dim() == 1
        check(self.L.rgbid_outlier_counts(self._h, self.ptr(out)))

    def emit(self, out):
        """write the kept records of the last plan into `out` (CUDA uint8 tensor [>= kept, 32]).  Asynchronous on the context's stream."""
        records_out(out)
        check(self.L.rgbid_outlier_emit(self._h, self.ptr(out), C.c_ulonglong(out.shape[0])))

    def filter(self, points, radius, min_neighbours, cap=None, return_counts=False, return_plan=False):
        """-> CUDA uint8 [kept, 32]: the records of at least min_neighbours neighbours within radius, unchanged, in input order; with
        return_counts also the int32 [M] counts (clamped at cap, as non-negative values below 2^31 or their two's complement above);
        with return_plan also the Plan.  `points` must stay unchanged until this returns (it synchronises)."""
        p = self.plan(points, radius, min_neighbours, cap)
        out = torch.empty((p.kept, 32), dtype=torch.uint8, device=self._dev)
        cnt = torch.empty((p.n,), dtype=torch.int32, device=self._dev) if return_counts else None
        self.ctx.wait_torch_stream()   # the outputs are torch's allocations
        if cnt is not None:
            self.counts(cnt)
        self.emit(out)
        self.ctx.sync()
        res = (out,) + ((cnt,) if return_counts else ()) + ((p,) if return_plan else ())
        return res if len(res) > 1 else out


def radius_filter(ctx, points, radius, min_neighbours, cap=None, return_counts=False, return_plan=False):
    """one-shot RadiusFilter(ctx, len(points)).filter(...); n = 0 does not touch the device"""
    if points.shape[0] == 0:
        radius32(radius); neighbour_args(min_neighbours, cap)
        out = torch.empty((0, 32), dtype=torch.uint8, device=points.device)
        cnt = torch.empty((0,), dtype=torch.int32, device=points.device)
        res = (out,) + ((cnt,) if return_counts else ()) + ((Plan(0, 0, np.zeros(3, np.uint64)),) if return_plan else ())
        return res if len(res) > 1 else out
    rf = RadiusFilter(ctx, points.shape[0])
    try:
        return rf.filter(points, radius, min_neighbours, cap, return_counts, return_plan)
    finally:
        rf.close()
