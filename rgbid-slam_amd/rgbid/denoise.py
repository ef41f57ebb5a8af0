"""Triangle meshes denoised on the device with their sharp edges kept (binding of include/rgbid_denoise.h).

`Denoiser.plan` builds the face table of the mesh (for every vertex the triangles with a corner at it, ascending); `Denoiser.normals`
computes the face normals and filters them over the faces that share a vertex with each, with the weight (n_i . n_j - T)^2 above the
threshold T and nothing below it, so that a face across a crease has no say; `Denoiser.vertices` moves the vertices along the normals of
their faces until those faces fit them (Sun, Rosin, Martin and Langbein, TVCG 2007); all byte-identical to the numpy restatement of the
contract.  `denoise_mesh` is the one-shot that `tsdf.Volume.extract` and `tsdf.fuse` call for their `denoise`
keyword."""
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
MAX_ITERATIONS = 256
SIGNATURES = {
    "rgbid_denoise_create": (vp, vp, u64, u64),
    "rgbid_denoise_destroy": (vp,),
    "rgbid_denoise_plan": (vp, u64, u64, vp, vp),
    "rgbid_denoise_faces": (vp, vp, vp),
    "rgbid_denoise_normals": (vp, vp, vp, cu, f64),
    "rgbid_denoise_vertices": (vp, vp, vp, vp, cu),
    "rgbid_denoise_timing": (vp, ci, vp),
}
EXPORTS = list(SIGNATURES)
STAGES = ("plan", "normals", "vertices")
COUNTS = ("empty_rows", "longest_row", "repeating_triangles", "work")


def capacity_arg(max_vertices, max_triangles):
    """-> (max_vertices, max_triangles) of a handle: 1 .. 2^31 and 1 .. 2^29 (ValueError otherwise)"""
    v, t = A.integer("max_vertices", max_vertices), A.integer("max_triangles", max_triangles)
    A.in_range("max_vertices", v, 1, MAX_VERTICES, "[1, 2^31]", max_vertices)
    return v, A.in_range("max_triangles", t, 1, MAX_TRIANGLES, "[1, 2^29]", max_triangles)


def mesh_arg(triangles, n_vertices, max_vertices=MAX_VERTICES, max_triangles=MAX_TRIANGLES, device=None):
    """-> (triangles, n_vertices): a contiguous CUDA tensor [n_t, 3] of 4-byte integers within the capacities, no triangles without vertices
    (ValueError otherwise)"""
    return MS.mesh_arg(triangles, n_vertices, max_vertices, max_triangles, device)


def iterations_arg(iterations, name="iterations"):
    """-> iterations: an integer in 0 .. 256 (ValueError otherwise)"""
    return A.integer_in(name, iterations, 0, MAX_ITERATIONS, f"[0, {MAX_ITERATIONS}]")


def threshold_arg(threshold):
    """-> threshold as a float: finite with 0 <= threshold < 1 (ValueError otherwise)"""
    if isinstance(threshold, (bool, str, bytes)) or not isinstance(threshold, (int, float, np.integer, np.floating)):
        raise ValueError(f"threshold: a number, got {threshold!r}")
    t = float(threshold)
    if not (math.isfinite(t) and 0.0 <= t < 1.0):
        raise ValueError(f"threshold must be finite with 0 <= threshold < 1, got {threshold!r}")
    return t


def denoise_arg(denoise):
    """-> None when denoise is None (no denoising), else dict(normal_iterations, vertex_iterations, threshold) as denoise_mesh takes them:
    denoise is a count of normal iterations, or a dict with normal_iterations and any of vertex_iterations (default 10) and threshold
    (default 0.4) (ValueError otherwise)"""
    if denoise is None:
        return None
    kw = dict(denoise) if isinstance(denoise, dict) else dict(normal_iterations=denoise)
    if "normal_iterations" not in kw or set(kw) - {"normal_iterations", "vertex_iterations", "threshold"}:
        raise ValueError(f"denoise: a count of normal iterations or a dict with normal_iterations and any of vertex_iterations, threshold, got {denoise!r}")
    return dict(normal_iterations=iterations_arg(kw["normal_iterations"], "normal_iterations"),
                vertex_iterations=iterations_arg(kw.get("vertex_iterations", 10), "vertex_iterations"), threshold=threshold_arg(kw.get("threshold", 0.4)))


class Denoiser(_lib.CtxHandle):
    """Feature-preserving denoising of meshes of up to max_vertices vertices and max_triangles triangles, on the context's stream."""
    _destroy, _signatures, _timing, _stages = "rgbid_denoise_destroy", SIGNATURES, "rgbid_denoise_timing", STAGES

    def __init__(self, ctx, max_vertices, max_triangles):
        self.max_vertices, self.max_triangles = capacity_arg(max_vertices, max_triangles)
        super().__init__(ctx)
        self._triangles = None                 # the planned triangles: the passes read them again
        self.n_vertices, self.n_triangles, self.counts = 0, 0, None
        self._created(self.L.rgbid_denoise_create(C.byref(self._h), ctx._h, C.c_ulonglong(self.max_vertices), C.c_ulonglong(self.max_triangles)))

    def plan(self, triangles, n_vertices):
        """the face table of the mesh `triangles` (CUDA [n_t, 3], 4-byte integers) over n_vertices vertices -> dict(empty_rows,
        longest_row, repeating_triangles, work).  The tensor is kept until the next plan: the passes read it.  Synchronises."""
        triangles, n_v = mesh_arg(triangles, n_vertices, self.max_vertices, self.max_triangles, self.ctx.device)
        self._triangles, self.counts = None, None
        counts = (C.c_ulonglong * 4)()
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_denoise_plan(self._h, C.c_ulonglong(n_v), C.c_ulonglong(triangles.shape[0]), self.ptr(triangles), counts))
        self._triangles, self.n_vertices, self.n_triangles = triangles, n_v, int(triangles.shape[0])
        self.counts = dict(zip(COUNTS, (int(x) for x in counts)))
        return dict(self.counts)

    def _planned(self, what):
        if self._triangles is None:
            raise ValueError(f"{what}: nothing is planned")

    def faces_into(self, offsets, faces):
        """the raw call: the last plan's CSR copied asynchronously on the context's stream into the given CUDA tensors (or None)"""
        check(self.L.rgbid_denoise_faces(self._h, self.opt_ptr(offsets), self.opt_ptr(faces)))

    def faces(self):
        """the last plan's CSR -> dict(offsets int32 [n_v + 1], faces int32 [3 n_t]) as new CUDA tensors (the int32 hold uint32 bits).
        Synchronises."""
        self._planned("faces")
        new = lambda rows: torch.empty((rows,), dtype=torch.int32, device=self._dev)
        out = dict(offsets=new(self.n_vertices + 1), faces=new(3 * self.n_triangles))
        self.ctx.wait_torch_stream()   # the outputs are torch's allocations
        self.faces_into(out["offsets"], out["faces"])
        self.ctx.sync()
        return out

    def normals_into(self, vertices, normals_out, iterations=5, threshold=0.4):
        """the raw call: the face normals of `vertices` (CUDA float32 [n_v, 3]) after `iterations` passes with `threshold` into
        normals_out (CUDA float32 [n_t, 3]), asynchronously on the context's stream"""
        n, t = iterations_arg(iterations), threshold_arg(threshold)
        self._planned("normals")
        A.rows3("vertices", vertices, torch.float32, self.n_vertices, self.ctx.device)
        A.rows3("normals_out", normals_out, torch.float32, None, self.ctx.device)
        if normals_out.shape[0] != self.n_triangles:
            raise ValueError(f"normals_out: {self.n_triangles} rows, one per triangle, got {normals_out.shape[0]}")
        check(self.L.rgbid_denoise_normals(self._h, self.ptr(vertices), self.ptr(normals_out), n, t))

    def normals(self, vertices, iterations=5, threshold=0.4):
        """the filtered face normals over the last plan -> a new CUDA tensor float32 [n_t, 3].  Synchronises."""
        n, t = iterations_arg(iterations), threshold_arg(threshold)
        self._planned("normals")
        A.rows3("vertices", vertices, torch.float32, self.n_vertices, self.ctx.device)
        out = torch.empty((self.n_triangles, 3), dtype=torch.float32, device=self._dev)
        self.ctx.wait_torch_stream()   # the output is torch's allocation
        self.normals_into(vertices, out, n, t)
        self.ctx.sync()
        return out

    def vertices_into(self, vertices, face_normals, vertices_out, iterations=10):
        """the raw call: `iterations` vertex passes from `vertices` into `vertices_out` (CUDA float32 [n_v, 3], not overlapping) with the
        normals `face_normals` (CUDA float32 [n_t, 3]), asynchronously on the context's stream"""
        n = iterations_arg(iterations)
        self._planned("vertices")
        for name, x in (("vertices", vertices), ("vertices_out", vertices_out)):
            A.rows3(name, x, torch.float32, self.n_vertices, self.ctx.device)
        A.rows3("face_normals", face_normals, torch.float32, None, self.ctx.device)
        if face_normals.shape[0] != self.n_triangles:
            raise ValueError(f"face_normals: {self.n_triangles} rows, one per triangle, got {face_normals.shape[0]}")
        check(self.L.rgbid_denoise_vertices(self._h, self.ptr(vertices), self.ptr(face_normals), self.ptr(vertices_out), n))

    def vertices(self, vertices, face_normals, iterations=10):
        """the positions after `iterations` vertex passes over the last plan -> a new CUDA tensor float32 [n_v, 3].  Synchronises."""
        n = iterations_arg(iterations)
        self._planned("vertices")
        A.rows3("vertices", vertices, torch.float32, self.n_vertices, self.ctx.device)
        out = torch.empty_like(vertices)
        self.ctx.wait_torch_stream()   # the output is torch's allocation
        self.vertices_into(vertices, face_normals, out, n)
        self.ctx.sync()
        return out

    def run(self, vertices, normal_iterations=5, vertex_iterations=10, threshold=0.4):
        """both stages over the last plan -> (positions float32 [n_v, 3], filtered face normals float32 [n_t, 3]).  Synchronises."""
        kw = denoise_arg(dict(normal_iterations=normal_iterations, vertex_iterations=vertex_iterations, threshold=threshold))
        nrm = self.normals(vertices, kw["normal_iterations"], kw["threshold"])
        return self.vertices(vertices, nrm, kw["vertex_iterations"]), nrm


def denoise_mesh(ctx, vertices, triangles, normal_iterations=5, vertex_iterations=10, threshold=0.4, normals=False):
    """one-shot: the mesh (vertices float32 [n, 3], triangles [n_t, 3], CUDA tensors) denoised -> (vertices, normals, info): the new
    positions, with `normals` the area-weighted vertex normals of the denoised surface from smooth.Smoother (None otherwise) and info =
    dict(vertices, triangles, normal_iterations, vertex_iterations, threshold, empty_rows, longest_row, repeating_triangles, work)."""
    kw = denoise_arg(dict(normal_iterations=normal_iterations, vertex_iterations=vertex_iterations, threshold=threshold))
    A.rows3("vertices", vertices, torch.float32)
    triangles, n_v = mesh_arg(triangles, vertices.shape[0])
    dn = Denoiser(ctx, max(n_v, 1), max(triangles.shape[0], 1))
    try:
        info = dn.plan(triangles, n_v)
        out, _ = dn.run(vertices, **kw)
    finally:
        dn.close()
    nrm = None
    if normals:
        from . import smooth as SO
        sm = SO.Smoother(ctx, max(n_v, 1), max(triangles.shape[0], 1))
        try:
            sm.plan(triangles, n_v, normals=True)
            nrm = sm.normals(out)
        finally:
            sm.close()
    info.update(vertices=n_v, triangles=int(triangles.shape[0]), **kw)
    return out, nrm, info
