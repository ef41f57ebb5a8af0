"""Mesh vertices recoloured from the keyframes that see them (binding of include/rgbid_recolour.h).

`Recolourer.add` projects every vertex of a mesh into further keyframes, keeps those that see it (not occluded against a surface-depth
plane, measured by the keyframe's own inverse depth, facing the camera), samples their colour planes bilinearly at full resolution and
accumulates the samples in integers; `Recolourer.finish` turns the sums into vertex colours, byte-identical to the numpy restatement of
the contract.  `recolour_mesh` is the one-shot over the keyframes of a run: it rasterises the mesh at every
keyframe's pose for the occlusion test and feeds the keyframes' own planes."""
import ctypes as C
import math

import numpy as np
import torch

from . import _args as A
from . import _lib
from . import raster as RS
from ._lib import check, ci, u64, vp
from .render import Pose, depth_range, intrinsics, poses

MAX_VERTICES = 1 << 31
MAX_VIEWS = 65535
MAX_DIM = RS.MAX_DIM
VIEW_CHUNK = 16
UNIT_WEIGHT = 1024
NO_VIEW = 0xFFFFFFFF
MODES = ("mean", "best")                # RGBID_RECOLOUR_MEAN, RGBID_RECOLOUR_BEST
SIGNATURES = {
    "rgbid_recolour_create": (vp, vp, u64),
    "rgbid_recolour_destroy": (vp,),
    "rgbid_recolour_begin": (vp, u64, ci),
    "rgbid_recolour_add": (vp, vp, vp, u64, ci, vp, vp, ci, ci, vp),
    "rgbid_recolour_finish": (vp, vp, vp, vp, vp),
    "rgbid_recolour_counts": (vp, ci, ci, vp),
    "rgbid_recolour_timing": (vp, ci, vp),
}
EXPORTS = list(SIGNATURES)
STAGES = ("accumulate", "resolve")
COUNTS = ("gated", "outside", "hidden", "unmeasured", "averted", "taken")


class View(C.Structure):
    """rgbid_recolour_view: a keyframe's world pose and its colour, surface-depth and inverse-depth planes"""
    _fields_ = [("pose", Pose), ("colour", C.c_void_p), ("surface", C.c_void_p), ("measured", C.c_void_p)]


class Params(C.Structure):
    """rgbid_recolour_params"""
    _fields_ = [("z_min", C.c_float), ("z_max", C.c_float), ("surface_tolerance", C.c_float), ("measured_tolerance", C.c_float),
                ("min_cos", C.c_float), ("two_sided", C.c_int)]


def capacity_arg(max_vertices):
    """-> the capacity of a handle: an integer in 1 .. 2^31 (ValueError otherwise)"""
    return A.integer_in("max_vertices", max_vertices, 1, MAX_VERTICES, "[1, 2^31]")


def count_arg(n_vertices, max_vertices=MAX_VERTICES):
    """-> the number of vertices of a begin: an integer in 0 .. the capacity (ValueError otherwise)"""
    return A.integer_in("n_vertices", n_vertices, 0, max_vertices, f"[0, {max_vertices}]")


def mode_arg(mode):
    """-> the mode as the library takes it: 0 for "mean", 1 for "best" (ValueError otherwise)"""
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"mode: one of {MODES}, got {mode!r}")
    return MODES.index(mode)


def tolerance_arg(name, v):
    """-> a tolerance in metres as the float32 value the library receives: finite and >= 0 (ValueError otherwise)"""
    f = A.float32(v, f"{name}: a number of metres, got {v!r}", (bool, str, bytes))
    if not (math.isfinite(f) and f >= 0):
        raise ValueError(f"{name} must be finite and >= 0, got {v!r}")
    return f


def cos_arg(min_cos):
    """-> min_cos as the float32 value the library receives: in [0, 1] (ValueError otherwise)"""
    f = A.float32(min_cos, f"min_cos: a number, got {min_cos!r}", (bool, str, bytes))
    if not 0 <= f <= 1:
        raise ValueError(f"min_cos must lie in [0, 1], got {min_cos!r}")
    return f


def flag_arg(name, v):
    """-> 0 or 1 for a bool, 0 or 1 (ValueError otherwise)"""
    if not (isinstance(v, (bool, np.bool_)) or (isinstance(v, (int, np.integer)) and v in (0, 1))):
        raise ValueError(f"{name}: True or False, got {v!r}")
    return int(v)


def image_size(rows, cols):
    """-> (rows, cols) as the library takes them: 1 .. 16384 each (ValueError otherwise)"""
    return RS.image_size(rows, cols)


def views_arg(views, begun=0):
    """-> the number of views of a call: at least 1, and with those since begin at most 65 535 (ValueError otherwise)"""
    v = A.integer("views", views)
    if v < 1:
        raise ValueError(f"at least one view, got {views!r}")
    if begun + v > MAX_VIEWS:
        raise ValueError(f"at most {MAX_VIEWS} views after one begin, got {begun} + {v}")
    return v


def vertices_arg(vertices, normals=None, rows=None, device=None):
    """-> (vertices, normals): contiguous CUDA float32 tensors [n_v, 3], of `rows` rows when given; normals may be None (ValueError
    otherwise)"""
    A.rows3("vertices", vertices, torch.float32, rows, device)
    if normals is not None:
        A.rows3("normals", normals, torch.float32, vertices.shape[0], device)
    return vertices, normals


def colour_planes_arg(colours, views, rows, cols, device=None):
    """-> the colour planes as a list of `views` contiguous CUDA uint8 tensors [rows, cols, 3] (ValueError otherwise).  colours: a
    sequence of such tensors (the keyframes' `colour`) or one tensor [views, rows, cols, 3]"""
    if isinstance(colours, torch.Tensor):
        colours = list(colours) if colours.dim() == 4 else [colours]
    try:
        colours = list(colours)
    except TypeError:
        raise ValueError("colours: a sequence of CUDA uint8 tensors [rows, cols, 3]") from None
    if len(colours) != views:
        raise ValueError(f"{views} views need {views} colour planes, got {len(colours)}")
    for c in colours:
        A.cuda_tensor("colours", c, torch.uint8, (rows, cols, 3), f"colours: contiguous CUDA uint8 tensors [{rows}, {cols}, 3]", device)
    return colours


def depth_planes_arg(name, planes, views, rows, cols, device=None):
    """-> None, or the float32 planes `name` as a list of `views` entries, each None or a contiguous CUDA float32 tensor [rows, cols]
    (ValueError otherwise).  planes: None, a sequence of such entries or one tensor [views, rows, cols]"""
    if planes is None:
        return [None] * views
    if isinstance(planes, torch.Tensor):
        planes = list(planes) if planes.dim() == 3 else [planes]
    try:
        planes = list(planes)
    except TypeError:
        raise ValueError(f"{name}: a sequence of CUDA float32 tensors [rows, cols] or None") from None
    if len(planes) != views:
        raise ValueError(f"{views} views need {views} {name} planes, got {len(planes)}")
    for p in planes:
        if p is not None:
            A.cuda_tensor(name, p, torch.float32, (rows, cols), f"{name}: contiguous CUDA float32 tensors [{rows}, {cols}] or None", device)
    return planes


def output_arg(name, x, dtype, shape, device=None):
    """-> x: None or a contiguous CUDA tensor of this dtype and shape (ValueError otherwise)"""
    if x is not None:
        A.cuda_tensor(name, x, dtype, shape, f"{name}: a contiguous CUDA {'int32' if dtype is A.int4 else str(dtype)[6:]} tensor {list(shape)}", device)
    return x


class Recolourer(_lib.CtxHandle):
    """The colouring of meshes of up to max_vertices vertices on the context's stream: begin, any number of add, finish.  timing() gives
    the last add's `accumulate` and the last finish's `resolve`."""
    _destroy, _signatures, _timing, _stages = "rgbid_recolour_destroy", SIGNATURES, "rgbid_recolour_timing", STAGES

    def __init__(self, ctx, max_vertices):
        self.max_vertices = capacity_arg(max_vertices)
        super().__init__(ctx)
        self.n_vertices, self.mode, self.views = None, None, 0
        self._held = []                       # what the stream may still read
        self._created(self.L.rgbid_recolour_create(C.byref(self._h), ctx._h, C.c_ulonglong(self.max_vertices)))

    def begin(self, n_vertices, mode="mean"):
        """clear the state for a mesh of n_vertices vertices (0 .. max_vertices); mode "mean": the weighted mean of all views that see a
        vertex, "best": the sample of the view that faces it most"""
        n, m = count_arg(n_vertices, self.max_vertices), mode_arg(mode)
        check(self.L.rgbid_recolour_begin(self._h, C.c_ulonglong(n), m))
        self.n_vertices, self.mode, self.views = n, mode, 0

    def add(self, vertices, R, t, K, rows, cols, colours, surface=None, depthinv=None, normals=None, z_min=0.05, z_max=20.0,
            surface_tolerance=0.02, measured_tolerance=0.02, min_cos=0.2, two_sided=False):
        """V further views of the mesh's vertices (CUDA float32 [n_v, 3], optional normals [n_v, 3]): world poses R [V, 3, 3], t [V, 3],
        K = fx, fy, cx, cy, the colour planes (CUDA uint8 [rows, cols, 3] each, or one tensor [V, rows, cols, 3]), optionally per view the
        mesh's depth at that pose (`surface`, float32 [rows, cols], NaN = empty: Rasteriser's depth plane) within surface_tolerance
        metres, and the keyframe's own inverse depth (`depthinv`) within measured_tolerance metres; a view whose normal makes a cosine
        below min_cos with the direction to the camera is left out (two_sided: the sign of the normal does not matter).  Asynchronous on
        the context's stream; the tensors are held until the next finish, counts or begin."""
        if self.n_vertices is None:
            raise ValueError("add: begin first")
        dev = self.ctx.device
        vertices_arg(vertices, normals, self.n_vertices, dev)
        R, t = poses(R, t)
        V = views_arg(len(R), self.views)
        rows, cols = image_size(rows, cols)
        k = (C.c_float * 4)(*intrinsics(K))
        colours = colour_planes_arg(colours, V, rows, cols, dev)
        surface = depth_planes_arg("surface", surface, V, rows, cols, dev)
        depthinv = depth_planes_arg("depthinv", depthinv, V, rows, cols, dev)
        lo, hi = depth_range(z_min, z_max)
        p = Params(lo, hi, tolerance_arg("surface_tolerance", surface_tolerance), tolerance_arg("measured_tolerance", measured_tolerance),
                   cos_arg(min_cos), flag_arg("two_sided", two_sided))
        ptr = lambda x: x.data_ptr() if x is not None else None
        arr = (View * V)(*[View(Pose((C.c_double * 9)(*R[v].reshape(9)), (C.c_double * 3)(*t[v])), ptr(colours[v]), ptr(surface[v]), ptr(depthinv[v]))
                           for v in range(V)])
        self.ctx.wait_torch_stream()          # the mesh and the planes were written on torch's stream
        check(self.L.rgbid_recolour_add(self._h, self.opt_ptr(vertices), self.opt_ptr(normals), C.c_ulonglong(vertices.shape[0]), V, arr, k, rows, cols,
                                        C.byref(p)))
        self._held += [vertices, normals, colours, surface, depthinv]
        self.views += V

    def finish_into(self, colours_in=None, colours_out=None, views_used=None, best_view=None):
        """the raw call: the given CUDA tensors (or None) filled asynchronously on the context's stream: colours uint8 [n_v, 3] (the
        output may be the input), views_used and best_view int32 [n_v] (uint32 bits)"""
        if self.n_vertices is None:
            raise ValueError("finish: begin first")
        n, dev = self.n_vertices, self.ctx.device
        output_arg("colours", colours_in, torch.uint8, (n, 3), dev)
        output_arg("colours_out", colours_out, torch.uint8, (n, 3), dev)
        output_arg("views_used", views_used, A.int4, (n,), dev)
        output_arg("best_view", best_view, A.int4, (n,), dev)
        if best_view is not None and self.mode != "best":
            raise ValueError("best_view: only after begin(mode=\"best\")")
        ptr = self.opt_ptr
        check(self.L.rgbid_recolour_finish(self._h, ptr(colours_in), ptr(colours_out), ptr(views_used), ptr(best_view)))

    def finish(self, colours=None):
        """the vertices' colours from the views added so far; `colours` (CUDA uint8 [n_v, 3], optional) is what a vertex keeps that no
        view was taken for (black without it) -> dict(colours uint8 [n_v, 3], views_used int32 [n_v], and in mode "best" best_view int32
        [n_v], -1 = none) as new CUDA tensors.  More views may be added afterwards.  Synchronises."""
        if self.n_vertices is None:
            raise ValueError("finish: begin first")
        n = self.n_vertices
        out = dict(colours=torch.empty((n, 3), dtype=torch.uint8, device=self._dev), views_used=torch.empty((n,), dtype=torch.int32, device=self._dev))
        if self.mode == "best":
            out["best_view"] = torch.empty((n,), dtype=torch.int32, device=self._dev)
        self.ctx.wait_torch_stream()          # the outputs are torch's allocations
        self.finish_into(colours, out["colours"], out["views_used"], out.get("best_view"))
        self.ctx.sync()
        self._held = []
        return out

    def counts(self, first=0, views=None):
        """the pairs per class of the views first .. first + views - 1 since begin (all of them by default) -> a list of dict(gated,
        outside, hidden, unmeasured, averted, taken), which sum to n_vertices.  Synchronises."""
        first = A.integer("first", first)
        views = self.views - first if views is None else A.integer("views", views)
        if first < 0 or views < 1 or first + views > self.views:
            raise ValueError(f"counts: views {first} .. {first + views - 1} of {self.views} added")
        out = (C.c_ulonglong * (6 * views))()
        check(self.L.rgbid_recolour_counts(self._h, first, views, out))
        self._held = []
        return [dict(zip(COUNTS, (int(x) for x in out[6 * v:6 * v + 6]))) for v in range(views)]


def counts_total(counts):
    """per-view counts -> their sum per class"""
    return {k: sum(c[k] for c in counts) for k in COUNTS}


def keyframes_arg(keyframes, measured):
    """-> the keyframes: a non-empty sequence of dicts with R, t and `colour`, and with `measured` also `depthinv` (ValueError otherwise)"""
    kfs = list(keyframes)
    if not kfs:
        raise ValueError("no keyframes to recolour from")
    for k in kfs:
        if k.get("colour") is None:
            raise ValueError("recolouring needs every keyframe's `colour` plane")
        if measured and k.get("depthinv") is None:
            raise ValueError("measured_tolerance needs every keyframe's `depthinv` plane")
    return kfs


def batch_arg(batch):
    """-> the keyframes rasterised at a time: an integer in 1 .. 4096 (ValueError otherwise)"""
    return A.integer_in("batch", batch, 1, RS.MAX_VIEWS, f"[1, {RS.MAX_VIEWS}]")


def recolour_mesh(ctx, vertices, triangles, keyframes, K, rows, cols, normals=None, colours=None, mode="mean", surface_tolerance=0.02,
                  measured_tolerance=None, min_cos=0.2, two_sided=False, z_min=0.05, z_max=20.0, batch=VIEW_CHUNK, timing=None):
    """The mesh (CUDA tensors: vertices float32 [n_v, 3], triangles [n_t, 3] of 4-byte integers, optional normals) coloured from the
    keyframes of a run (dicts with the world pose R, t and the `colour` plane, CUDA uint8 [rows, cols, 3]): the mesh is rasterised at
    `batch` keyframe poses at a time and a keyframe colours a vertex only where the mesh's own depth at the vertex's pixel footprint
    agrees with the vertex's within surface_tolerance metres (no other part of the mesh is in front); with measured_tolerance also only
    where the keyframe's own `depthinv` agrees.  colours: what a vertex keeps that no keyframe sees -> (colours uint8 [n_v, 3],
    views_used int32 [n_v], counts: per keyframe dict(gated, outside, hidden, unmeasured, averted, taken)).  timing: a dict that
    receives the summed device ms of `raster`, `accumulate` and `resolve`."""
    RS.mesh_arg(vertices, triangles, colours, normals)
    kfs = keyframes_arg(keyframes, measured_tolerance is not None)
    mode_arg(mode); cos_arg(min_cos); flag_arg("two_sided", two_sided); depth_range(z_min, z_max); intrinsics(K)
    tolerance_arg("surface_tolerance", surface_tolerance)
    if measured_tolerance is not None:
        tolerance_arg("measured_tolerance", measured_tolerance)
    rows, cols = image_size(rows, cols)
    batch = min(batch_arg(batch), len(kfs))
    views_arg(len(kfs))
    n_v = vertices.shape[0]
    rs = RS.Rasteriser(ctx, max(n_v, 1), max(triangles.shape[0], 1), rows * cols * batch)
    rc = None
    try:
        rc = Recolourer(ctx, max(n_v, 1))
        if timing is not None:
            rs.timing(True); rc.timing(True)
            timing.update(raster=0.0, accumulate=0.0, resolve=0.0)
        rc.begin(n_v, mode)
        depth = torch.empty((batch, rows, cols), dtype=torch.float32, device=rc._dev)
        for a in range(0, len(kfs), batch):
            part = kfs[a:a + batch]
            R, t = np.stack([np.asarray(k["R"]) for k in part]), np.stack([np.asarray(k["t"]) for k in part])
            ctx.wait_torch_stream()
            rs.render_into(vertices, triangles, R, t, K, rows, cols, None, None, z_min, z_max, depth=depth[:len(part)])
            rc.add(vertices, R, t, K, rows, cols, [k["colour"] for k in part], depth[:len(part)],
                   [k["depthinv"] for k in part] if measured_tolerance is not None else None, normals, z_min, z_max, surface_tolerance,
                   0.0 if measured_tolerance is None else measured_tolerance, min_cos, two_sided)
            if timing is not None:
                ctx.sync()
                timing["raster"] += sum(rs.timing(True).values())
                timing["accumulate"] += rc.timing(True)["accumulate"]
        out = rc.finish(colours)
        if timing is not None:
            timing["resolve"] = rc.timing(True)["resolve"]
        return out["colours"], out["views_used"], rc.counts()
    finally:
        if rc is not None:
            rc.close()
        rs.close()
