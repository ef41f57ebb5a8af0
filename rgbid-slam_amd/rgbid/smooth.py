"""Triangle meshes smoothed by Taubin's lambda | mu filter on the device, and area-weighted vertex normals (binding of
include/rgbid_smooth.h).

`Smoother.plan` builds the umbrella neighbourhoods of the vertices from the triangles (a CSR of the distinct neighbours in ascending order,
how many triangle corners join each pair, which vertices lie on a boundary) and, for normals, the corners of every vertex; `Smoother.run`
moves the vertices (each iteration a pass with lambda and, unless mu is 0, one with mu; ordered double sums); `Smoother.normals` sums the
area vectors of a vertex's triangles; all byte-identical to the numpy restatement of the contract.  `smooth_mesh` is
the one-shot that `tsdf.Volume.extract` and `tsdf.fuse` call for their `smooth` keyword."""
import ctypes as C
import math

import numpy as np
import torch

from . import _args as A
from . import _lib
from . import mesh as MS
from ._lib import check, ci, cu, f64, u64, vp

MAX_VERTICES = 1 << 31
MAX_TRIANGLES = 1 << 29
MAX_ITERATIONS = 4096
PLAN_NORMALS = 1
PIN_BOUNDARY = 1
SIGNATURES = {
    "rgbid_smooth_create": (vp, vp, u64, u64),
    "rgbid_smooth_destroy": (vp,),
    "rgbid_smooth_plan": (vp, u64, u64, vp, cu, vp),
    "rgbid_smooth_adjacency": (vp, vp, vp, vp, vp, u64),
    "rgbid_smooth_run": (vp, vp, vp, cu, f64, f64, cu),
    "rgbid_smooth_normals": (vp, vp, vp),
    "rgbid_smooth_timing": (vp, ci, vp),
}
EXPORTS = list(SIGNATURES)
STAGES = ("plan", "run", "normals")
COUNTS = ("pairs", "edges", "boundary_pairs", "boundary_vertices", "isolated", "max_degree", "dropped", "non_manifold")


def capacity_arg(max_vertices, max_triangles):
    """-> (max_vertices, max_triangles) of a handle: 1 .. 2^31 and 1 .. 2^29 (ValueError otherwise)"""
    v, t = A.integer("max_vertices", max_vertices), A.integer("max_triangles", max_triangles)
    A.in_range("max_vertices", v, 1, MAX_VERTICES, "[1, 2^31]", max_vertices)
    return v, A.in_range("max_triangles", t, 1, MAX_TRIANGLES, "[1, 2^29]", max_triangles)


def mesh_arg(triangles, n_vertices, max_vertices=MAX_VERTICES, max_triangles=MAX_TRIANGLES, device=None):
    """-> (triangles, n_vertices): a contiguous CUDA tensor [n_t, 3] of 4-byte integers within the capacities, no triangles without vertices
    (ValueError otherwise)"""
    return MS.mesh_arg(triangles, n_vertices, max_vertices, max_triangles, device)


def iterations_arg(iterations):
    """-> iterations: an integer in 0 .. 4096 (ValueError otherwise)"""
    return A.integer_in("iterations", iterations, 0, MAX_ITERATIONS, f"[0, {MAX_ITERATIONS}]")


def factors_arg(lam, mu):
    """-> (lambda, mu) as floats: lambda finite with 0 < lambda <= 1, mu finite with -2 <= mu <= 0 (ValueError otherwise)"""
    for name, x in (("lam", lam), ("mu", mu)):
        if isinstance(x, (bool, str, bytes)) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name}: a number, got {x!r}")
    lam, mu = float(lam), float(mu)
    if not (math.isfinite(lam) and 0.0 < lam <= 1.0):
        raise ValueError(f"lam must be finite with 0 < lam <= 1, got {lam!r}")
    if not (math.isfinite(mu) and -2.0 <= mu <= 0.0):
        raise ValueError(f"mu must be finite with -2 <= mu <= 0, got {mu!r}")
    return lam, mu


class Smoother(_lib.CtxHandle):
    """Taubin smoothing and vertex normals of meshes of up to max_vertices vertices and max_triangles triangles, on the context's stream."""
    _destroy, _signatures, _timing, _stages = "rgbid_smooth_destroy", SIGNATURES, "rgbid_smooth_timing", STAGES

    def __init__(self, ctx, max_vertices, max_triangles):
        self.max_vertices, self.max_triangles = capacity_arg(max_vertices, max_triangles)
        super().__init__(ctx)
        self._triangles = None                 # the planned triangles: normals reads them again
        self.n_vertices, self.counts, self.has_normals = 0, None, False
        self._created(self.L.rgbid_smooth_create(C.byref(self._h), ctx._h, C.c_ulonglong(self.max_vertices), C.c_ulonglong(self.max_triangles)))

    def plan(self, triangles, n_vertices, normals=False):
        """the neighbourhoods of the mesh `triangles` (CUDA [n_t, 3], 4-byte integers) over n_vertices vertices, with `normals` also the
        corner table -> dict(pairs, edges, boundary_pairs, boundary_vertices, isolated, max_degree, dropped, non_manifold).  The tensor is
        kept until the next plan: normals reads it.  Synchronises."""
        triangles, n_v = mesh_arg(triangles, n_vertices, self.max_vertices, self.max_triangles, self.ctx.device)
        self._triangles, self.counts = None, None
        counts = (C.c_ulonglong * 8)()
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_smooth_plan(self._h, C.c_ulonglong(n_v), C.c_ulonglong(triangles.shape[0]), self.ptr(triangles), PLAN_NORMALS if normals else 0,
                                       counts))
        self._triangles, self.n_vertices, self.has_normals = triangles, n_v, bool(normals)
        self.counts = dict(zip(COUNTS, (int(x) for x in counts)))
        return dict(self.counts)

    def _planned(self, what):
        if self._triangles is None:
            raise ValueError(f"{what}: nothing is planned")

    def adjacency_into(self, offsets, neighbours, incidences, boundary, pair_capacity):
        """the raw call: the last plan's CSR copied asynchronously on the context's stream into the given CUDA tensors (or None)"""
        ptr = self.opt_ptr
        check(self.L.rgbid_smooth_adjacency(self._h, ptr(offsets), ptr(neighbours), ptr(incidences), ptr(boundary), C.c_ulonglong(pair_capacity)))

    def adjacency(self):
        """the last plan's CSR -> dict(offsets int32 [n_v + 1], neighbours int32 [P], incidences int32 [P], boundary uint8 [n_v]) as new
        CUDA tensors (the int32 hold uint32 bits).  Synchronises."""
        self._planned("adjacency")
        p, n = self.counts["pairs"], self.n_vertices
        new = lambda rows, dtype=torch.int32: torch.empty((rows,), dtype=dtype, device=self._dev)
        out = dict(offsets=new(n + 1), neighbours=new(p), incidences=new(p), boundary=new(n, torch.uint8))
        self.ctx.wait_torch_stream()   # the outputs are torch's allocations
        self.adjacency_into(out["offsets"], out["neighbours"], out["incidences"], out["boundary"], p)
        self.ctx.sync()
        return out

    def run_into(self, vertices, vertices_out, iterations, lam=0.5, mu=-0.53, pin_boundary=False):
        """the raw call: `iterations` iterations from `vertices` into `vertices_out` (CUDA float32 [n_v, 3], not overlapping),
        asynchronously on the context's stream"""
        n = iterations_arg(iterations)
        lam, mu = factors_arg(lam, mu)
        self._planned("run")
        for name, x in (("vertices", vertices), ("vertices_out", vertices_out)):
            A.rows3(name, x, torch.float32, self.n_vertices, self.ctx.device)
        check(self.L.rgbid_smooth_run(self._h, self.ptr(vertices), self.ptr(vertices_out), n, lam, mu, PIN_BOUNDARY if pin_boundary else 0))

    def run(self, vertices, iterations, lam=0.5, mu=-0.53, pin_boundary=False):
        """the positions after `iterations` iterations over the last plan -> a new CUDA tensor float32 [n_v, 3].  Synchronises."""
        n = iterations_arg(iterations)
        lam, mu = factors_arg(lam, mu)
        self._planned("run")
        A.rows3("vertices", vertices, torch.float32, self.n_vertices, self.ctx.device)
        out = torch.empty_like(vertices)
        self.ctx.wait_torch_stream()   # the output is torch's allocation
        self.run_into(vertices, out, n, lam, mu, pin_boundary)
        self.ctx.sync()
        return out

    def normals_into(self, vertices, normals_out):
        """the raw call: the area-weighted normals of `vertices` over the last plan into normals_out, asynchronously"""
        check(self.L.rgbid_smooth_normals(self._h, self.ptr(vertices), self.ptr(normals_out)))

    def normals(self, vertices):
        """the area-weighted unit normals of the positions `vertices` (CUDA float32 [n_v, 3]) over the last plan, which must have been made
        with normals=True -> a new CUDA tensor float32 [n_v, 3] (0 0 0 where the area vectors cancel or there is none).  Synchronises."""
        self._planned("normals")
        if not self.has_normals:
            raise ValueError("normals: the plan was made without normals=True")
        A.rows3("vertices", vertices, torch.float32, self.n_vertices, self.ctx.device)
        out = torch.empty_like(vertices)
        self.ctx.wait_torch_stream()   # the output is torch's allocation
        self.normals_into(vertices, out)
        self.ctx.sync()
        return out


def smooth_mesh(ctx, vertices, triangles, iterations, lam=0.5, mu=-0.53, pin_boundary=False, normals=False):
    """one-shot: the mesh (vertices float32 [n, 3], triangles [n_t, 3], CUDA tensors) after `iterations` Taubin iterations -> (vertices,
    normals, info): the new positions, with `normals` the area-weighted normals of the smoothed surface (None otherwise) and info =
    dict(vertices, triangles, iterations, lam, mu, pin_boundary, pairs, edges, boundary_pairs, boundary_vertices, isolated, max_degree,
    dropped, non_manifold)."""
    n = iterations_arg(iterations)
    lam, mu = factors_arg(lam, mu)
    A.rows3("vertices", vertices, torch.float32)
    triangles, n_v = mesh_arg(triangles, vertices.shape[0])
    sm = Smoother(ctx, max(n_v, 1), max(triangles.shape[0], 1))
    try:
        info = sm.plan(triangles, n_v, normals=normals)
        out = sm.run(vertices, n, lam, mu, pin_boundary)
        nrm = sm.normals(out) if normals else None
    finally:
        sm.close()
    info.update(vertices=n_v, triangles=int(triangles.shape[0]), iterations=n, lam=lam, mu=mu, pin_boundary=bool(pin_boundary))
    return out, nrm, info
