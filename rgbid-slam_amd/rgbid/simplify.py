"""Triangle meshes simplified by vertex clustering on the device (binding of include/rgbid_simplify.h).

`Simplifier.plan` lays the voxel filter's grid over the vertices, makes every occupied cell a cluster and classifies the triangles rewritten
over the clusters (lost, collapsed, duplicate, kept); `Simplifier.emit` writes one representative per cluster (the mean position, the
rounded mean colour, the normalised sum of the normals) and the kept triangles; all byte-identical to the numpy restatement of the contract
(DESIGN.md section 23).  `simplify_mesh` is the one-shot that `tsdf.Volume.extract` and `tsdf.fuse` call for their `simplify` keyword."""
import ctypes as C

import numpy as np
import torch

from . import _args as A
from . import _lib
from . import mesh as MS
from ._lib import check, ci, cu, u64, vp

MAX_VERTICES = 1 << 31
MAX_TRIANGLES = 1 << 31
NO_CLUSTER = 0xFFFFFFFF
KEEP_DUPLICATES = 1
SIGNATURES = {
    "rgbid_simplify_create": (vp, vp, u64, u64),
    "rgbid_simplify_destroy": (vp,),
    "rgbid_simplify_plan": (vp, u64, vp, u64, vp, vp, cu, vp, vp),
    "rgbid_simplify_emit": (vp, vp, vp, vp, vp, vp, vp, vp, vp, u64, u64),
    "rgbid_simplify_timing": (vp, ci, vp),
}
EXPORTS = list(SIGNATURES)
STAGES = ("vertices", "triangles", "emit")
COUNTS = ("participating", "clusters", "lost", "collapsed", "duplicate", "kept")

capacity_arg = MS.capacity_arg


def cell_arg(cell):
    """-> (c0, c1, c2): the cell edges in metres as float32 values, from a scalar or three values; each finite and > 0 as a float32
    (ValueError otherwise)"""
    try:
        if isinstance(cell, (bool, str, bytes)) or isinstance(cell, torch.Tensor):
            raise TypeError
        with np.errstate(over="ignore"):
            c = np.asarray(cell, dtype=np.float64).astype(np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"cell: a number of metres or three of them, got {cell!r}") from None
    if c.shape == ():
        c = np.repeat(c, 3)
    if c.shape != (3,):
        raise ValueError(f"cell: a number of metres or three of them, got {cell!r}")
    if not (np.isfinite(c).all() and (c > 0).all()):
        raise ValueError(f"cell: every edge finite and > 0 in float32, got {cell!r}")
    return tuple(float(x) for x in c)


def mesh_arg(vertices, triangles, max_vertices=MAX_VERTICES, max_triangles=MAX_TRIANGLES, device=None):
    """-> (vertices, triangles): contiguous CUDA tensors float32 [n_v, 3] and 4-byte integers [n_t, 3] within the capacities, no triangles
    without vertices (ValueError otherwise)"""
    A.rows3("vertices", vertices, torch.float32, device=device)
    triangles, _ = MS.mesh_arg(triangles, vertices.shape[0], max_vertices, max_triangles, device)
    return vertices, triangles


class Simplifier(_lib.CtxHandle):
    """Vertex clustering of meshes of up to max_vertices vertices and max_triangles triangles, on the context's stream."""
    _destroy, _signatures, _timing, _stages = "rgbid_simplify_destroy", SIGNATURES, "rgbid_simplify_timing", STAGES

    def __init__(self, ctx, max_vertices, max_triangles):
        self.max_vertices, self.max_triangles = capacity_arg(max_vertices, max_triangles)
        super().__init__(ctx)
        self._mesh = None                      # the planned mesh: emit reads it again
        self.counts = None
        self._created(self.L.rgbid_simplify_create(C.byref(self._h), ctx._h, C.c_ulonglong(self.max_vertices), C.c_ulonglong(self.max_triangles)))

    def plan(self, vertices, triangles, cell, keep_duplicates=False):
        """cluster the mesh (CUDA float32 [n_v, 3], 4-byte integers [n_t, 3]) with cells of `cell` metres (a scalar or three values)
        -> dict(grid = min_b[3] + div_b[3], participating, clusters, lost, collapsed, duplicate, kept).  Both tensors are kept until the
        next plan: emit reads them.  Synchronises."""
        cell = cell_arg(cell)
        vertices, triangles = mesh_arg(vertices, triangles, self.max_vertices, self.max_triangles, self.ctx.device)
        self._mesh, self.counts = None, None
        grid, counts = (C.c_longlong * 6)(), (C.c_ulonglong * 6)()
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_simplify_plan(self._h, C.c_ulonglong(vertices.shape[0]), self.ptr(vertices), C.c_ulonglong(triangles.shape[0]),
                                         self.ptr(triangles), (C.c_float * 3)(*cell), KEEP_DUPLICATES if keep_duplicates else 0, grid, counts))
        self._mesh = (vertices, triangles)
        self.counts = dict(zip(COUNTS, (int(x) for x in counts)))
        return dict(grid=[int(x) for x in grid], **self.counts)

    def emit_into(self, colours, normals, vertices_out, colours_out, normals_out, members_out, cluster_of_out, triangles_out):
        """the raw call: the last plan written asynchronously on the context's stream into the given CUDA tensors (or None)"""
        ptr = self.opt_ptr
        rows = lambda x: C.c_ulonglong(x.shape[0] if x is not None else 0)
        check(self.L.rgbid_simplify_emit(self._h, ptr(colours), ptr(normals), ptr(vertices_out), ptr(colours_out), ptr(normals_out), ptr(members_out),
                                         ptr(cluster_of_out), ptr(triangles_out), rows(vertices_out), rows(triangles_out)))

    def emit(self, colours=None, normals=None, members=False, cluster_of=False):
        """the last plan's mesh, optionally with the vertices' colours (uint8 [n_v, 3]) and normals (float32 [n_v, 3]) -> dict(vertices,
        colours, normals, triangles, members, cluster_of) as new CUDA tensors (None where there was no input or it was not asked for;
        members int32 [C], cluster_of int32 [n_v] holding uint32 bits).  Synchronises."""
        if self._mesh is None:
            raise ValueError("emit: nothing is planned")
        dev, n = self.ctx.device, self._mesh[0].shape[0]
        if colours is not None:
            A.rows3("colours", colours, torch.uint8, n, dev)
        if normals is not None:
            A.rows3("normals", normals, torch.float32, n, dev)
        nc, kt = self.counts["clusters"], self.counts["kept"]
        new = lambda like, rows: None if like is None else torch.empty((rows, 3), dtype=like.dtype, device=self._dev)
        out = dict(vertices=new(self._mesh[0], nc), colours=new(colours, nc), normals=new(normals, nc),
                   triangles=torch.empty((kt, 3), dtype=torch.int32, device=self._dev),
                   members=torch.empty((nc,), dtype=torch.int32, device=self._dev) if members else None,
                   cluster_of=torch.empty((n,), dtype=torch.int32, device=self._dev) if cluster_of else None)
        self.ctx.wait_torch_stream()   # the outputs are torch's allocations
        self.emit_into(colours, normals, out["vertices"], out["colours"], out["normals"], out["members"], out["cluster_of"], out["triangles"])
        self.ctx.sync()
        return out


def simplify_mesh(ctx, vertices, colours, triangles, normals=None, cell=0.05, keep_duplicates=False, drop_unreferenced=True):
    """one-shot: the mesh (vertices float32 [n, 3], colours uint8 [n, 3] or None, triangles [n_t, 3], normals float32 [n, 3] or None, CUDA
    tensors) clustered with cells of `cell` metres; with drop_unreferenced the clusters that no kept triangle names are then removed by
    mesh.filter_components(min_triangles=1) -> (vertices, colours, triangles, normals, info) with info = dict(grid, vertices, triangles,
    participating, clusters, lost, collapsed, duplicate, kept, out_vertices, out_triangles)."""
    cell = cell_arg(cell)
    vertices, triangles = mesh_arg(vertices, triangles)
    sp = Simplifier(ctx, max(vertices.shape[0], 1), max(triangles.shape[0], 1))
    try:
        info = sp.plan(vertices, triangles, cell, keep_duplicates)
        out = sp.emit(colours, normals)
    finally:
        sp.close()
    v, c, t, n = out["vertices"], out["colours"], out["triangles"], out["normals"]
    if drop_unreferenced:
        v, c, t, n, _ = MS.filter_components(ctx, v, c, t, n, min_triangles=1)
    info.update(vertices=int(vertices.shape[0]), triangles=int(triangles.shape[0]), out_vertices=int(v.shape[0]), out_triangles=int(t.shape[0]))
    return v, c, t, n, info
