"""Small holes of triangle meshes closed on the device (binding of include/rgbid_holes.h).

`Filler.plan` finds the boundary half-edges of the triangles (the edges that one corner names), the vertices that one of them leaves and
one enters, and the closed loops of those; `Filler.select` gives every loop a status from the positions (too long, not finite, an outline
whose cap would face against its rim, filled); `Filler.emit` writes the mesh with one new vertex at the centre of every filled loop and a
fan of triangles around it; all byte-identical to the numpy restatement of the contract.  `fill_holes` is the
one-shot that `tsdf.Volume.extract` and `tsdf.fuse` call for their `fill_holes` keyword."""
import ctypes as C

import numpy as np
import torch

from . import _args as A
from . import _lib
from . import mesh as MS
from ._lib import check, ci, cu, u64, vp

MAX_VERTICES = 1 << 31
MAX_TRIANGLES = 1 << 29
MIN_EDGES = 3
MAX_EDGES = (1 << 31) - 1
ANY_FACING = 1
FILLED, TOO_LONG, NOT_FINITE, OUTLINE = 0, 1, 2, 3
SIGNATURES = {
    "rgbid_holes_create": (vp, vp, u64, u64),
    "rgbid_holes_destroy": (vp,),
    "rgbid_holes_plan": (vp, u64, u64, vp, vp),
    "rgbid_holes_loops": (vp, vp, vp, vp, vp, u64),
    "rgbid_holes_select": (vp, vp, cu, cu, vp),
    "rgbid_holes_emit": (vp, vp, vp, vp, vp, vp, vp, vp, vp, u64, u64),
    "rgbid_holes_timing": (vp, ci, vp),
}
EXPORTS = list(SIGNATURES)
STAGES = ("plan", "select", "emit")
PLAN_COUNTS = ("directed_edges", "boundary_half_edges", "boundary_vertices", "non_simple", "loops", "loop_edges", "blocked", "longest")
SELECT_COUNTS = ("too_long", "not_finite", "outlines", "filled", "new_triangles")


def capacity_arg(max_vertices, max_triangles):
    """-> (max_vertices, max_triangles) of a handle: 1 .. 2^31 and 1 .. 2^29 (ValueError otherwise)"""
    v, t = A.integer("max_vertices", max_vertices), A.integer("max_triangles", max_triangles)
    A.in_range("max_vertices", v, 1, MAX_VERTICES, "[1, 2^31]", max_vertices)
    return v, A.in_range("max_triangles", t, 1, MAX_TRIANGLES, "[1, 2^29]", max_triangles)


def mesh_arg(triangles, n_vertices, max_vertices=MAX_VERTICES, max_triangles=MAX_TRIANGLES, device=None):
    """-> (triangles, n_vertices): a contiguous CUDA tensor [n_t, 3] of 4-byte integers within the capacities, no triangles without vertices
    (ValueError otherwise)"""
    return MS.mesh_arg(triangles, n_vertices, max_vertices, max_triangles, device)


def max_edges_arg(max_edges):
    """-> max_edges: an integer in 3 .. 2^31 - 1, the longest loop that is filled (ValueError otherwise)"""
    return A.integer_in("max_edges", max_edges, MIN_EDGES, MAX_EDGES, "[3, 2^31 - 1]")


def attributes_arg(vertices, colours, normals, n_vertices, device=None):
    """-> (vertices, colours, normals): contiguous CUDA tensors [n_vertices, 3], float32, uint8 or None, float32 or None (ValueError
    otherwise)"""
    A.rows3("vertices", vertices, torch.float32, n_vertices, device)
    if colours is not None:
        A.rows3("colours", colours, torch.uint8, n_vertices, device)
    if normals is not None:
        A.rows3("normals", normals, torch.float32, n_vertices, device)
    return vertices, colours, normals


def fill_holes_arg(fill_holes):
    """what tsdf.Volume.extract and tsdf.fuse take for their `fill_holes` keyword -> None when it is None (no filling), else dict(max_edges,
    any_facing) as fill_holes takes them: the longest loop to close, an integer in 3 .. 2^31 - 1, or a dict with `max_edges` and optionally
    any_facing (default False) (ValueError otherwise)"""
    if fill_holes is None:
        return None
    kw = dict(fill_holes) if isinstance(fill_holes, dict) else dict(max_edges=fill_holes)
    unknown = sorted(set(kw) - {"max_edges", "any_facing"})
    if unknown or "max_edges" not in kw:
        raise ValueError(f"fill_holes: a loop length or a dict with max_edges and optionally any_facing, got {fill_holes!r}")
    facing = kw.get("any_facing", False)
    if not isinstance(facing, (bool, np.bool_)):
        raise ValueError(f"fill_holes: any_facing is True or False, got {facing!r}")
    return dict(max_edges=max_edges_arg(kw["max_edges"]), any_facing=bool(facing))


class Filler(_lib.CtxHandle):
    """The boundary loops of meshes of up to max_vertices vertices and max_triangles triangles and their caps, on the context's stream."""
    _destroy, _signatures, _timing, _stages = "rgbid_holes_destroy", SIGNATURES, "rgbid_holes_timing", STAGES

    def __init__(self, ctx, max_vertices, max_triangles):
        self.max_vertices, self.max_triangles = capacity_arg(max_vertices, max_triangles)
        super().__init__(ctx)
        self._triangles = None                 # the planned triangles: select reads them again
        self.n_vertices, self.counts, self.selected = 0, None, None
        self._created(self.L.rgbid_holes_create(C.byref(self._h), ctx._h, C.c_ulonglong(self.max_vertices), C.c_ulonglong(self.max_triangles)))

    def plan(self, triangles, n_vertices):
        """the loops of the mesh `triangles` (CUDA [n_t, 3], 4-byte integers) over n_vertices vertices -> dict(directed_edges,
        boundary_half_edges, boundary_vertices, non_simple, loops, loop_edges, blocked, longest).  The tensor is kept until the next plan:
        select reads it.  Synchronises."""
        triangles, n_v = mesh_arg(triangles, n_vertices, self.max_vertices, self.max_triangles, self.ctx.device)
        self._triangles, self.counts, self.selected = None, None, None
        counts = (C.c_ulonglong * 8)()
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_holes_plan(self._h, C.c_ulonglong(n_v), C.c_ulonglong(triangles.shape[0]), self.ptr(triangles), counts))
        self._triangles, self.n_vertices = triangles, n_v
        self.counts = dict(zip(PLAN_COUNTS, (int(x) for x in counts)))
        return dict(self.counts)

    def _planned(self, what):
        if self._triangles is None:
            raise ValueError(f"{what}: nothing is planned")

    def _selected(self, what):
        self._planned(what)
        if self.selected is None:
            raise ValueError(f"{what}: nothing is selected")

    def loops_into(self, offsets, vertices, owners, status, capacity):
        """the raw call: the last plan's loop table copied asynchronously on the context's stream into the given CUDA tensors (or None)"""
        ptr = self.opt_ptr
        check(self.L.rgbid_holes_loops(self._h, ptr(offsets), ptr(vertices), ptr(owners), ptr(status), C.c_ulonglong(capacity)))

    def loops(self, status=False):
        """the last plan's loop table -> dict(offsets int32 [L + 1], vertices int32 [S], owners int32 [S]) as new CUDA tensors (the int32
        hold uint32 bits), with `status` also status uint8 [L], which needs a select.  Synchronises."""
        self._selected("loops") if status else self._planned("loops")
        n_l, s = self.counts["loops"], self.counts["loop_edges"]
        new = lambda rows, dtype=torch.int32: torch.empty((rows,), dtype=dtype, device=self._dev)
        out = dict(offsets=new(n_l + 1), vertices=new(s), owners=new(s))
        if status:
            out["status"] = new(n_l, torch.uint8)
        self.ctx.wait_torch_stream()   # the outputs are torch's allocations
        self.loops_into(out["offsets"], out["vertices"], out["owners"], out.get("status"), s)
        self.ctx.sync()
        return out

    def select(self, vertices, max_edges=64, any_facing=False):
        """the status of every loop of the last plan from the positions `vertices` (CUDA float32 [n_v, 3]): loops of more than max_edges
        edges are too long, a loop with a position that is not finite is left, a loop whose cap would face against its rim's triangles is
        an outline unless `any_facing` -> dict(too_long, not_finite, outlines, filled, new_triangles).  Synchronises."""
        k = max_edges_arg(max_edges)
        self._planned("select")
        A.rows3("vertices", vertices, torch.float32, self.n_vertices, self.ctx.device)
        self.selected = None
        counts = (C.c_ulonglong * 5)()
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_holes_select(self._h, self.ptr(vertices), k, ANY_FACING if any_facing else 0, counts))
        self.selected = dict(zip(SELECT_COUNTS, (int(x) for x in counts)))
        return dict(self.selected)

    def emit_into(self, vertices, colours, normals, triangles, vertices_out, colours_out, normals_out, triangles_out):
        """the raw call: the last selection written asynchronously on the context's stream into the given CUDA tensors (or None)"""
        ptr = self.opt_ptr
        check(self.L.rgbid_holes_emit(self._h, ptr(vertices), ptr(colours), ptr(normals), ptr(triangles), ptr(vertices_out), ptr(colours_out),
                                      ptr(normals_out), ptr(triangles_out), C.c_ulonglong(vertices_out.shape[0]), C.c_ulonglong(triangles_out.shape[0])))

    def emit(self, vertices, triangles, colours=None, normals=None):
        """the mesh with the filled loops of the last selection closed -> dict(vertices, colours, normals, triangles) as new CUDA tensors
        (None where there was no input).  `triangles` is the planned mesh's tensor.  Synchronises."""
        self._selected("emit")
        dev, n = self.ctx.device, self.n_vertices
        attributes_arg(vertices, colours, normals, n, dev)
        A.rows3("triangles", triangles, A.int4, self._triangles.shape[0], dev)
        rows_v, rows_t = n + self.selected["filled"], triangles.shape[0] + self.selected["new_triangles"]
        new = lambda like, rows: None if like is None else torch.empty((rows, 3), dtype=like.dtype, device=self._dev)
        out = dict(vertices=new(vertices, rows_v), colours=new(colours, rows_v), normals=new(normals, rows_v), triangles=new(triangles, rows_t))
        self.ctx.wait_torch_stream()   # the outputs are torch's allocations
        self.emit_into(vertices, colours, normals, triangles, out["vertices"], out["colours"], out["normals"], out["triangles"])
        self.ctx.sync()
        return out


def fill_holes(ctx, vertices, colours, triangles, normals, max_edges=64, any_facing=False):
    """one-shot: the mesh (vertices float32 [n, 3], colours uint8 [n, 3] or None, triangles [n_t, 3], normals float32 [n, 3] or None, CUDA
    tensors) with its loops of at most max_edges edges closed -> (vertices, colours, triangles, normals, figures) with figures = the eight
    counts of the plan and the five of the selection."""
    k = max_edges_arg(max_edges)
    A.rows3("vertices", vertices, torch.float32)
    triangles, n_v = mesh_arg(triangles, vertices.shape[0])
    attributes_arg(vertices, colours, normals, n_v)
    fl = Filler(ctx, max(n_v, 1), max(triangles.shape[0], 1))
    try:
        figures = fl.plan(triangles, n_v)
        figures.update(fl.select(vertices, k, any_facing))
        out = fl.emit(vertices, triangles, colours, normals)
        return out["vertices"], out["colours"], out["triangles"], out["normals"], figures
    finally:
        fl.close()
