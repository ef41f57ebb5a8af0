"""Voxel-grid filter over keyframe point clouds (binding of include/rgbid_voxel.h).

The reference writes its map through pcl::VoxelGrid with a 1 cm leaf (savePointCloudInFile, tools/RGBID_SLAMapp.cpp:341-354): every
occupied cell becomes the centroid of its points.  `VoxelGrid.build` does that on the device over the 32-byte records of `rgbid.cloud`
and returns one record per voxel, in ascending cell-key order, bitwise reproducible.  The voxel records have the
cloud records' offsets, with the member count where the cloud record holds its pixel, so `rgbid.cloud.write_ply` writes them unchanged.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ci, cu, u64, vp
from .cloud import records, records_out

# rgbid_voxel_point: centroid, mean normal, member count, mean colour, flags (bit 0: some member is novel)
VOXEL_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("count", "<u4"),
                        ("r", "u1"), ("g", "u1"), ("b", "u1"), ("flags", "u1")])
assert VOXEL_DTYPE.itemsize == 32

MAX_POINTS = 1 << 31
SIGNATURES = {
    "rgbid_voxel_create": (vp, vp, u64),
    "rgbid_voxel_destroy": (vp,),
    "rgbid_voxel_plan": (vp, vp, u64, vp, cu, vp, vp, vp),
    "rgbid_voxel_emit": (vp, vp, u64),
    "rgbid_voxel_timing": (vp, ci, vp),
}
EXPORTS = list(SIGNATURES)
STAGES = ("box", "keys", "sort", "runs", "emit")


def leaf3(leaf):
    """a scalar or 3 leaf sizes -> 3 float32 values, each finite and > 0 (ValueError otherwise)"""
    v = [float(leaf)] * 3 if np.ndim(leaf) == 0 else [float(x) for x in leaf]
    if len(v) != 3:
        raise ValueError(f"leaf: a scalar or 3 values, got {leaf!r}")
    f = [float(np.float32(x)) for x in v]
    if not all(math.isfinite(x) and x > 0 for x in f):
        raise ValueError(f"leaf sizes must be finite and > 0, got {leaf!r}")
    return f


def as_numpy(voxels):
    """[V, 32] uint8 records (a device or host tensor, or a numpy array) -> structured array of VOXEL_DTYPE"""
    a = voxels.cpu().numpy() if isinstance(voxels, torch.Tensor) else np.asarray(voxels)
    return np.ascontiguousarray(a).view(VOXEL_DTYPE).reshape(-1)


class Plan:
    """what rgbid_voxel_plan reports: voxels (records the emit writes), grid min_b[3] / div_b[3], finite points, voxels before and after
    min_points"""

    def __init__(self, voxels, grid, stats):
        self.voxels = int(voxels)
        self.min_b, self.div_b = [int(x) for x in grid[:3]], [int(x) for x in grid[3:]]
        self.finite, self.runs, self.kept = [int(x) for x in stats]

    def __repr__(self):
        return (f"Plan(voxels={self.voxels}, min_b={self.min_b}, div_b={self.div_b}, finite={self.finite}, runs={self.runs}, "
                f"kept={self.kept})")


class VoxelGrid(_lib.CtxHandle):
    """Voxel-grid filter for up to max_points input records per plan, on the context's stream."""
    _destroy, _signatures, _timing, _stages = "rgbid_voxel_destroy", SIGNATURES, "rgbid_voxel_timing", STAGES

    def __init__(self, ctx, max_points):
        super().__init__(ctx)
        self.max_points = int(max_points)
        self._created(self.L.rgbid_voxel_create(C.byref(self._h), ctx._h, C.c_ulonglong(self.max_points)))

    def plan(self, points, leaf=0.01, min_points=0):
        """grid, sort and count pass over `points` (CUDA uint8 [M, 32] rgbid_cloud_point records) -> Plan.  Synchronises (on the context's
        stream: records written on torch's stream are waited for first)."""
        records(points)
        lf = (C.c_float * 3)(*leaf3(leaf))
        grid = np.zeros(6, np.int64); stats = np.zeros(3, np.uint64); nv = C.c_ulonglong()
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_voxel_plan(self._h, self.ptr(points), C.c_ulonglong(points.shape[0]), lf,
                                      C.c_uint(int(min_points)), grid.ctypes.data_as(C.c_void_p), stats.ctypes.data_as(C.c_void_p), C.byref(nv)))
        return Plan(nv.value, grid, stats)

    def emit(self, out):
        """write the voxels of the last plan into `out` (CUDA uint8 tensor [>= V, 32]).  Asynchronous on the context's stream."""
        records_out(out)
        check(self.L.rgbid_voxel_emit(self._h, self.ptr(out), C.c_ulonglong(out.shape[0])))

    def build(self, points, leaf=0.01, min_points=0, return_plan=False):
        """-> CUDA uint8 [V, 32] of rgbid_voxel_point records (as_numpy gives the structured view); with return_plan, (voxels, Plan).
        `points` must stay unchanged until this returns (it synchronises)."""
        p = self.plan(points, leaf, min_points)
        out = torch.empty((p.voxels, 32), dtype=torch.uint8, device=self._dev)
        self.ctx.wait_torch_stream()   # the output is torch's allocation
        self.emit(out)
        self.ctx.sync()
        return (out, p) if return_plan else out


def voxel_grid(ctx, points, leaf=0.01, min_points=0, return_plan=False):
    """one-shot VoxelGrid(ctx, len(points)).build(points, leaf, min_points)"""
    if points.shape[0] == 0:
        out = torch.empty((0, 32), dtype=torch.uint8, device=points.device)
        leaf3(leaf)
        return (out, Plan(0, np.zeros(6, np.int64), np.zeros(3, np.uint64))) if return_plan else out
    vg = VoxelGrid(ctx, points.shape[0])
    try:
        return vg.build(points, leaf, min_points, return_plan)
    finally:
        vg.close()
