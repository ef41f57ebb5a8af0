"""Triangle meshes refined on the device by splitting their long edges (binding of include/rgbid_refine.h).

`Refiner.plan` builds the table of the distinct edges of the triangles, marks those of the selected triangles that are longer than
`max_edge` and counts what a split of them gives; `Refiner.emit` writes the mesh with one new vertex at the midpoint of every marked edge
and every triangle cut by the pattern of its marked edges (one, two, three or four children, the orientation kept, no T-junction); all
byte-identical to the numpy restatement of the contract.  One plan and emit halve the marked edges;
`refine_mesh` is the one-shot that repeats them until no edge is too long, and what `tsdf.Volume.extract` and `tsdf.fuse` call for their
`refine` keyword."""
import ctypes as C

import numpy as np
import torch

from . import _args as A
from . import _lib
from . import mesh as MS
from ._lib import check, ci, f64, u64, vp

MAX_VERTICES = 1 << 31
MAX_TRIANGLES = 1 << 29
MAX_ROUNDS = 16
SIGNATURES = {
    "rgbid_refine_create": (vp, vp, u64, u64),
    "rgbid_refine_destroy": (vp,),
    "rgbid_refine_plan": (vp, u64, u64, vp, vp, vp, f64, vp),
    "rgbid_refine_emit": (vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u64, u64),
    "rgbid_refine_timing": (vp, ci, vp),
}
EXPORTS = list(SIGNATURES)
STAGES = ("plan", "emit")
PLAN_COUNTS = ("edges", "eligible", "marked", "k0", "k1", "k2", "k3", "degenerate", "new_triangles")


def capacity_arg(max_vertices, max_triangles):
    """-> (max_vertices, max_triangles) of a handle: 1 .. 2^31 and 1 .. 2^29 (ValueError otherwise)"""
    v, t = A.integer("max_vertices", max_vertices), A.integer("max_triangles", max_triangles)
    A.in_range("max_vertices", v, 1, MAX_VERTICES, "[1, 2^31]", max_vertices)
    return v, A.in_range("max_triangles", t, 1, MAX_TRIANGLES, "[1, 2^29]", max_triangles)


def mesh_arg(triangles, n_vertices, max_vertices=MAX_VERTICES, max_triangles=MAX_TRIANGLES, device=None):
    """-> (triangles, n_vertices): a contiguous CUDA tensor [n_t, 3] of 4-byte integers within the capacities, no triangles without vertices
    (ValueError otherwise)"""
    return MS.mesh_arg(triangles, n_vertices, max_vertices, max_triangles, device)


def max_edge_arg(max_edge):
    """-> max_edge as a float: a finite length >= 0, no bool and no str (ValueError otherwise)"""
    f = A.finite64("max_edge", max_edge)
    if f < 0:
        raise ValueError(f"max_edge must be a finite length >= 0, got {max_edge!r}")
    return f


def rounds_arg(rounds):
    """-> rounds: an integer in 0 .. 16, the most plan-and-emit rounds of refine_mesh (ValueError otherwise)"""
    return A.integer_in("rounds", rounds, 0, MAX_ROUNDS, "[0, 16]")


def selection_arg(selection, n_triangles, device=None):
    """-> selection: None (every triangle) or a contiguous CUDA uint8 tensor [n_triangles] (ValueError otherwise)"""
    if selection is None:
        return None
    A.cuda_tensor("selection", selection, torch.uint8, (None,), "selection: a contiguous CUDA uint8 tensor [n_t]", device)
    if selection.shape[0] != n_triangles:
        raise ValueError(f"selection: {n_triangles} bytes, one per triangle, got {selection.shape[0]}")
    return selection


def attributes_arg(vertices, colours, normals, n_vertices, device=None):
    """-> (vertices, colours, normals): contiguous CUDA tensors [n_vertices, 3], float32, uint8 or None, float32 or None (ValueError
    otherwise)"""
    A.rows3("vertices", vertices, torch.float32, n_vertices, device)
    if colours is not None:
        A.rows3("colours", colours, torch.uint8, n_vertices, device)
    if normals is not None:
        A.rows3("normals", normals, torch.float32, n_vertices, device)
    return vertices, colours, normals


def refine_arg(refine):
    """what tsdf.Volume.extract and tsdf.fuse take for their `refine` keyword -> None when it is None (no refinement), else dict(max_edge,
    rounds, caps_only): refine is the longest edge to keep in metres, or a dict with `max_edge` and optionally rounds (default 4) and
    caps_only (default False: with True only the fans that fill_holes appended are selected) (ValueError otherwise)"""
    if refine is None:
        return None
    kw = dict(refine) if isinstance(refine, dict) else dict(max_edge=refine)
    unknown = sorted(set(kw) - {"max_edge", "rounds", "caps_only"})
    if unknown or "max_edge" not in kw:
        raise ValueError(f"refine: a length or a dict with max_edge and optionally rounds, caps_only, got {refine!r}")
    caps = kw.get("caps_only", False)
    if not isinstance(caps, (bool, np.bool_)):
        raise ValueError(f"refine: caps_only is True or False, got {caps!r}")
    return dict(max_edge=max_edge_arg(kw["max_edge"]), rounds=rounds_arg(kw.get("rounds", 4)), caps_only=bool(caps))


class Refiner(_lib.CtxHandle):
    """One round of the edge split of meshes of up to max_vertices vertices and max_triangles triangles, on the context's stream."""
    _destroy, _signatures, _timing, _stages = "rgbid_refine_destroy", SIGNATURES, "rgbid_refine_timing", STAGES

    def __init__(self, ctx, max_vertices, max_triangles):
        self.max_vertices, self.max_triangles = capacity_arg(max_vertices, max_triangles)
        super().__init__(ctx)
        self.n_vertices, self.n_triangles, self.counts = 0, 0, None
        self._created(self.L.rgbid_refine_create(C.byref(self._h), ctx._h, C.c_ulonglong(self.max_vertices), C.c_ulonglong(self.max_triangles)))

    def plan(self, triangles, vertices, max_edge, selection=None):
        """the edges of the mesh `triangles` (CUDA [n_t, 3], 4-byte integers) over the positions `vertices` (CUDA float32 [n_v, 3]) that
        are longer than max_edge and belong to a triangle with a non-zero byte in `selection` (CUDA uint8 [n_t]; None: every triangle)
        -> dict(edges, eligible, marked, k0, k1, k2, k3, degenerate, new_triangles).  Synchronises."""
        length = max_edge_arg(max_edge)
        A.rows3("vertices", vertices, torch.float32, None, self.ctx.device)
        triangles, n_v = mesh_arg(triangles, vertices.shape[0], self.max_vertices, self.max_triangles, self.ctx.device)
        selection_arg(selection, triangles.shape[0], self.ctx.device)
        self.counts = None
        counts = (C.c_ulonglong * 9)()
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_refine_plan(self._h, C.c_ulonglong(n_v), C.c_ulonglong(triangles.shape[0]), self.ptr(triangles), self.ptr(vertices),
                                       self.opt_ptr(selection), length, counts))
        self.n_vertices, self.n_triangles = n_v, int(triangles.shape[0])
        self.counts = dict(zip(PLAN_COUNTS, (int(x) for x in counts)))
        return dict(self.counts)

    def _planned(self, what):
        if self.counts is None:
            raise ValueError(f"{what}: nothing is planned")

    def emit_into(self, vertices, colours, normals, triangles, selection, vertices_out, colours_out, normals_out, triangles_out, selection_out):
        """the raw call: the last plan written asynchronously on the context's stream into the given CUDA tensors (or None)"""
        ptr = self.opt_ptr
        check(self.L.rgbid_refine_emit(self._h, ptr(vertices), ptr(colours), ptr(normals), ptr(triangles), ptr(selection), ptr(vertices_out),
                                       ptr(colours_out), ptr(normals_out), ptr(triangles_out), ptr(selection_out),
                                       C.c_ulonglong(vertices_out.shape[0]), C.c_ulonglong(triangles_out.shape[0])))

    def emit(self, vertices, triangles, colours=None, normals=None, selection=None):
        """the planned mesh with its marked edges split -> dict(vertices, colours, normals, triangles, selection) as new CUDA tensors (None
        where there was no input).  Synchronises."""
        self._planned("emit")
        dev, n = self.ctx.device, self.n_vertices
        attributes_arg(vertices, colours, normals, n, dev)
        A.rows3("triangles", triangles, A.int4, self.n_triangles, dev)
        selection_arg(selection, self.n_triangles, dev)
        rows_v, rows_t = n + self.counts["marked"], self.n_triangles + self.counts["new_triangles"]
        new = lambda like, rows: None if like is None else torch.empty((rows,) + tuple(like.shape[1:]), dtype=like.dtype, device=self._dev)
        out = dict(vertices=new(vertices, rows_v), colours=new(colours, rows_v), normals=new(normals, rows_v), triangles=new(triangles, rows_t),
                   selection=new(selection, rows_t))
        self.ctx.wait_torch_stream()   # the outputs are torch's allocations
        self.emit_into(vertices, colours, normals, triangles, selection, out["vertices"], out["colours"], out["normals"], out["triangles"],
                       out["selection"])
        self.ctx.sync()
        return out


def refine_mesh(ctx, vertices, colours, triangles, normals, max_edge, rounds=4, selection=None):
    """one-shot: the mesh (vertices float32 [n, 3], colours uint8 [n, 3] or None, triangles [n_t, 3], normals float32 [n, 3] or None,
    selection uint8 [n_t] or None, CUDA tensors) with the edges of its selected triangles above max_edge split, in at most `rounds` plan-
    and-emit rounds: it stops at the first plan without a marked edge and plans once more when the rounds ran out -> (vertices, colours,
    triangles, normals, selection, figures) with figures = dict(max_edge, rounds = the nine counts of every round that was emitted,
    rounds_run, left = the edges still above max_edge, vertices, triangles).  The handle is sized for the round's input and replaced by one
    at least twice as large when a round outgrows it."""
    length, most = max_edge_arg(max_edge), rounds_arg(rounds)
    A.rows3("vertices", vertices, torch.float32)
    triangles, n_v = mesh_arg(triangles, vertices.shape[0])
    attributes_arg(vertices, colours, normals, n_v)
    selection_arg(selection, triangles.shape[0])
    v, c, t, n, s = vertices, colours, triangles, normals, selection
    rf, per_round, left = None, [], 0
    try:
        for i in range(most + 1):
            if rf is None or v.shape[0] > rf.max_vertices or t.shape[0] > rf.max_triangles:
                if rf is not None:
                    rf.close()
                grow = 1 if rf is None else 2
                rf = Refiner(ctx, min(max(grow * v.shape[0], 1), MAX_VERTICES), min(max(grow * t.shape[0], 1), MAX_TRIANGLES))
            counts = rf.plan(t, v, length, s)
            left = counts["marked"]
            if left == 0 or i == most:
                break
            per_round.append(counts)
            out = rf.emit(v, t, c, n, s)
            v, c, t, n, s = out["vertices"], out["colours"], out["triangles"], out["normals"], out["selection"]
    finally:
        if rf is not None:
            rf.close()
    return v, c, t, n, s, dict(max_edge=length, rounds=per_round, rounds_run=len(per_round), left=left, vertices=int(v.shape[0]),
                               triangles=int(t.shape[0]))


def cap_selection(n_before, n_after, device):
    """the selection of `caps_only`: the triangles n_before .. n_after - 1 that holes.fill_holes appended -> CUDA uint8 [n_after]"""
    s = torch.zeros((n_after,), dtype=torch.uint8, device=device)
    s[n_before:] = 1
    return s
