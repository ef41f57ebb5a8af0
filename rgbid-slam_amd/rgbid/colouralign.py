"""Keyframe poses refined against the colours of a mesh (binding of include/rgbid_colouralign.h).

`ColourAligner.run` alternates, on the device and without a host wait, the grey value every mesh vertex should have (the weighted mean
over the keyframes that see it) and one 6-DoF Gauss-Newton step per keyframe that moves its image onto those values, byte-identical to
tests/colouralign_mirror.py.  `refine_keyframes` is the one-shot over the keyframes of a run, coarse to fine: it
gives back the keyframes with refined poses for `recolour.recolour_mesh` and `texture` to sample.  No geometry changes."""
import ctypes as C

import numpy as np
import torch

from . import _args as A
from . import _lib
from . import raster as RS
from . import recolour as RC
from ._lib import check, ci, u64, vp
from .render import Pose, depth_range, intrinsics, poses

MAX_VERTICES = 1 << 31
MAX_VIEWS = 2048
MAX_ITERATIONS = 256
MAX_FACTOR = 16
TERMS = 28
RUNNING, CONVERGED, FEW, SINGULAR, FIXED = 0, 1, 2, 3, 4
STATUS = ("running", "converged", "few", "singular", "fixed")                                                        # RGBID_COLOURALIGN_*
SIGNATURES = {
    "rgbid_colouralign_create": (vp, vp, u64, ci),
    "rgbid_colouralign_destroy": (vp,),
    "rgbid_colouralign_run": (vp, vp, vp, u64, ci, vp, vp, ci, ci, vp, vp, vp),
    "rgbid_colouralign_targets": (vp, vp, vp, vp),
    "rgbid_colouralign_set_target_form": (vp, ci),
    "rgbid_colouralign_timing": (vp, ci, vp),
    "rgbid_colouralign_downscale": (vp, vp, ci, ci, ci, vp),
}
EXPORTS = list(SIGNATURES)
STAGES = ("target", "system", "solve")
TARGET_FORMS = ("auto", "walk", "chunks")                 # RGBID_COLOURALIGN_TARGET_*
# rgbid_colouralign_result: 560 bytes
RESULT = np.dtype([("pose", "<f8", (12,)), ("status", "<i4"), ("iterations", "<i4"), ("used", "<u4", (2,)), ("sums", "<f8", (2, TERMS))])


class View(C.Structure):
    """rgbid_colouralign_view"""
    _fields_ = [("view", RC.View), ("fixed", C.c_int)]


class Rule(C.Structure):
    """rgbid_colouralign_rule"""
    _fields_ = [("huber", C.c_float), ("damping", C.c_double), ("eps", C.c_double), ("min_pairs", C.c_uint), ("min_views", C.c_uint),
                ("rounds", C.c_int), ("iterations", C.c_int), ("stride", C.c_int)]


def capacity_arg(max_vertices, max_views):
    """-> the capacities of a handle: max_vertices in 1 .. 2^31, max_views in 1 .. 2048 (ValueError otherwise)"""
    return (A.integer_in("max_vertices", max_vertices, 1, MAX_VERTICES, "[1, 2^31]"),
            A.integer_in("max_views", max_views, 1, MAX_VIEWS, f"[1, {MAX_VIEWS}]"))


def views_arg(views, max_views=MAX_VIEWS):
    """-> the number of views of a call: 1 .. the capacity (ValueError otherwise)"""
    return A.integer_in("views", views, 1, max_views, f"[1, {max_views}]")


def fixed_arg(fixed, views):
    """-> the sorted indices of the views whose pose is held: None or a sequence of distinct integers in 0 .. views - 1 (ValueError
    otherwise)"""
    if fixed is None:
        return ()
    try:
        idx = [A.integer("fixed", i) for i in fixed]
    except TypeError:
        raise ValueError(f"fixed: a sequence of view indices, got {fixed!r}") from None
    if len(set(idx)) != len(idx) or any(not 0 <= i < views for i in idx):
        raise ValueError(f"fixed: distinct view indices in [0, {views - 1}], got {fixed!r}")
    return tuple(sorted(idx))


def rule_arg(huber, damping, eps, min_pairs, min_views, rounds, iterations, stride):
    """-> the rule as the library takes it: huber a finite float32 > 0 (grey levels), damping finite and >= 0, eps finite and > 0,
    min_pairs >= 6, min_views >= 2, rounds, iterations and stride >= 1, rounds * iterations <= 256 (ValueError otherwise)"""
    h, d, e = A.finite32("huber", huber), A.finite64("damping", damping), A.finite64("eps", eps)
    if not h > 0:
        raise ValueError(f"huber must be > 0, got {huber!r}")
    if not d >= 0:
        raise ValueError(f"damping must be >= 0, got {damping!r}")
    if not e > 0:
        raise ValueError(f"eps must be > 0, got {eps!r}")
    mp = A.integer_in("min_pairs", min_pairs, 6, (1 << 32) - 1, "[6, 2^32 - 1]")
    mv = A.integer_in("min_views", min_views, 2, (1 << 32) - 1, "[2, 2^32 - 1]")
    r = A.integer_in("rounds", rounds, 1, MAX_ITERATIONS, f"[1, {MAX_ITERATIONS}]")
    i = A.integer_in("iterations", iterations, 1, MAX_ITERATIONS, f"[1, {MAX_ITERATIONS}]")
    if r * i > MAX_ITERATIONS:
        raise ValueError(f"rounds * iterations must be at most {MAX_ITERATIONS}, got {rounds!r} * {iterations!r}")
    s = A.integer_in("stride", stride, 1, (1 << 31) - 1, "[1, 2^31 - 1]")
    return h, d, e, mp, mv, r, i, s


def target_form_arg(form):
    """-> the target pass's form as the library takes it: 0 for "auto", 1 for "walk", 2 for "chunks" (ValueError otherwise)"""
    if not isinstance(form, str) or form not in TARGET_FORMS:
        raise ValueError(f"form: one of {TARGET_FORMS}, got {form!r}")
    return TARGET_FORMS.index(form)


def scales_arg(scales, rows, cols):
    """-> the scales of refine_keyframes as a tuple: 1 .. 8 integers in 1 .. 16, each leaving at least one row and one column
    (ValueError otherwise)"""
    try:
        sc = tuple(A.integer("scales", f) for f in scales)
    except TypeError:
        raise ValueError(f"scales: a sequence of integers, got {scales!r}") from None
    if not 1 <= len(sc) <= 8 or any(not 1 <= f <= MAX_FACTOR or rows // f < 1 or cols // f < 1 for f in sc):
        raise ValueError(f"scales: 1 .. 8 factors in [1, {MAX_FACTOR}] that leave a row and a column, got {scales!r}")
    return sc


def scaled_intrinsics(K, f):
    """K at 1 / f of the resolution, a pixel's centre at u = p: (fx / f, fy / f, (cx - (f - 1) / 2) / f, (cy - (f - 1) / 2) / f)"""
    fx, fy, cx, cy = intrinsics(K)
    return fx / f, fy / f, (cx - (f - 1) / 2.0) / f, (cy - (f - 1) / 2.0) / f


def result_dict(res):
    """the records of rgbid_colouralign_run (RESULT [V]) -> dict(R [V, 3, 3], t [V, 3], status, iterations [V], used [V, 2],
    H [V, 2, 6, 6], b [V, 2, 6], error [V, 2], records: the RESULT array); index 0 of the pairs is the first system built, 1 the last"""
    H = np.zeros((len(res), 2, 6, 6), np.float64)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            H[:, :, i, j] = H[:, :, j, i] = res["sums"][:, :, k]
            k += 1
    return dict(R=res["pose"][:, :9].reshape(-1, 3, 3).copy(), t=res["pose"][:, 9:].copy(), status=res["status"].copy(),
                iterations=res["iterations"].copy(), used=res["used"].copy(), H=H, b=res["sums"][:, :, 21:27].copy(),
                error=res["sums"][:, :, 27].copy(), records=res.copy())


def cost_per_pair(result):
    """the weighted squared grey residual per used pair of the first and of the last system of every view of a `run` result, float64
    [V, 2], NaN where no pair was used"""
    with np.errstate(all="ignore"):
        return np.asarray(result["error"]) / np.asarray(result["used"]).astype(np.float64)


class ColourAligner(_lib.CtxHandle):
    """The pose refinement of up to max_views views of meshes of up to max_vertices vertices, on the context's stream.  timing() gives
    the last run's `target`, `system` and `solve`, summed over its rounds and iterations."""
    _destroy, _signatures, _timing, _stages = "rgbid_colouralign_destroy", SIGNATURES, "rgbid_colouralign_timing", STAGES

    def __init__(self, ctx, max_vertices, max_views):
        self.max_vertices, self.max_views = capacity_arg(max_vertices, max_views)
        super().__init__(ctx)
        self.lattice = None                   # the last run's lattice size
        self._held = []                       # what the stream may still read
        self._created(self.L.rgbid_colouralign_create(C.byref(self._h), ctx._h, C.c_ulonglong(self.max_vertices), self.max_views))

    def target_form(self, form="auto"):
        """how the following runs walk the target pass: "walk" (all views per vertex), "chunks" (chunks of 16 views over blocks, integer
        atomics) or "auto" (the library's choice by the lattice and the views, the default); the results are the same"""
        check(self.L.rgbid_colouralign_set_target_form(self._h, target_form_arg(form)))

    def run_into(self, result, vertices, R, t, K, rows, cols, colours, surface=None, depthinv=None, normals=None, fixed=(0,), huber=16.0,
                 damping=0.0, eps=1e-7, min_pairs=6, min_views=2, rounds=4, iterations=3, stride=1, z_min=0.05, z_max=20.0,
                 surface_tolerance=0.02, measured_tolerance=0.02, min_cos=0.2, two_sided=False):
        """the raw call: checked arguments, the records written asynchronously on the context's stream into `result`, a contiguous CUDA
        uint8 tensor of 560 bytes per view; the tensors are held until the next run"""
        dev = self.ctx.device
        A.rows3("vertices", vertices, torch.float32, device=dev)
        if vertices.shape[0] > self.max_vertices:
            raise ValueError(f"{vertices.shape[0]} vertices are more than the handle's {self.max_vertices}")
        RC.vertices_arg(vertices, normals, vertices.shape[0], dev)
        R, t = poses(R, t)
        V = views_arg(len(R), self.max_views)
        fixed = fixed_arg(fixed, V)
        rows, cols = RC.image_size(rows, cols)
        k = (C.c_float * 4)(*intrinsics(K))
        colours = RC.colour_planes_arg(colours, V, rows, cols, dev)
        surface = RC.depth_planes_arg("surface", surface, V, rows, cols, dev)
        depthinv = RC.depth_planes_arg("depthinv", depthinv, V, rows, cols, dev)
        lo, hi = depth_range(z_min, z_max)
        p = RC.Params(lo, hi, RC.tolerance_arg("surface_tolerance", surface_tolerance), RC.tolerance_arg("measured_tolerance", measured_tolerance),
                      RC.cos_arg(min_cos), RC.flag_arg("two_sided", two_sided))
        rule = Rule(*rule_arg(huber, damping, eps, min_pairs, min_views, rounds, iterations, stride))
        if not (isinstance(result, torch.Tensor) and result.is_cuda and result.dtype == torch.uint8 and result.is_contiguous()
                and result.numel() == V * RESULT.itemsize and result.device.index == dev and result.data_ptr() % 8 == 0):
            raise ValueError(f"result: a contiguous CUDA uint8 tensor of {V} x {RESULT.itemsize} bytes on device {dev}")
        ptr = lambda x: x.data_ptr() if x is not None else None
        arr = (View * V)(*[View(RC.View(Pose((C.c_double * 9)(*R[v].reshape(9)), (C.c_double * 3)(*t[v])), ptr(colours[v]), ptr(surface[v]),
                                        ptr(depthinv[v])), int(v in fixed)) for v in range(V)])
        self.ctx.wait_torch_stream()          # the mesh and the planes were written on torch's stream
        check(self.L.rgbid_colouralign_run(self._h, self.opt_ptr(vertices), self.opt_ptr(normals), C.c_ulonglong(vertices.shape[0]), V, arr, k, rows,
                                           cols, C.byref(p), C.byref(rule), C.c_void_p(result.data_ptr())))
        self._held = [vertices, normals, colours, surface, depthinv, result]
        self.lattice = (vertices.shape[0] + rule.stride - 1) // rule.stride
        return V

    def run(self, vertices, R, t, K, rows, cols, colours, **kw):
        """refine the world poses R [V, 3, 3], t [V, 3] of V views of the mesh's vertices (CUDA float32 [n, 3], optional `normals`): K =
        fx, fy, cx, cy, the colour planes (CUDA uint8 [rows, cols, 3] each), optionally per view the mesh's depth at the starting pose
        (`surface`: Rasteriser's depth plane) and the keyframe's own inverse depth (`depthinv`), with the gates of Recolourer.add
        (z_min, z_max, surface_tolerance, measured_tolerance, min_cos, two_sided).  fixed: the views whose pose is held (the first by
        default; None: none).  rounds target passes, each followed by `iterations` Gauss-Newton steps per view over every stride-th vertex,
        with the Huber threshold `huber` in grey levels, the damping H_jj (1 + damping), the step bound `eps`, at least `min_pairs` used
        pairs per view and `min_views` views per vertex -> dict(R, t float64, status [V] (an index into STATUS), iterations [V],
        used [V, 2], H [V, 2, 6, 6], b [V, 2, 6], error [V, 2], records).  Synchronises."""
        V = len(poses(R, t)[0])
        result = torch.empty((V * RESULT.itemsize,), dtype=torch.uint8, device=self._dev)
        self.run_into(result, vertices, R, t, K, rows, cols, colours, **kw)
        self.ctx.sync()
        self._held = []
        return result_dict(result.cpu().numpy().view(RESULT))

    def targets_into(self, S=None, W=None, used=None):
        """the raw call: the last run's last target pass over its lattice into the given CUDA tensors (or None): S and W int64 [n_l]
        (uint64 bits), used int32 [n_l] (uint32 bits).  Asynchronous on the context's stream."""
        if self.lattice is None:
            raise ValueError("targets: run first")
        n, dev = self.lattice, self.ctx.device
        for name, x, dtype in (("S", S, torch.int64), ("W", W, torch.int64), ("used", used, A.int4)):
            if x is not None:
                A.cuda_tensor(name, x, dtype, (n,), f"{name}: a contiguous CUDA tensor [{n}] of {'4' if dtype is A.int4 else '8'}-byte integers", dev)
        check(self.L.rgbid_colouralign_targets(self._h, self.opt_ptr(S), self.opt_ptr(W), self.opt_ptr(used)))

    def targets(self):
        """the last run's last target pass over its lattice -> dict(S, W int64 (uint64 bits) [n_l], used int32 (uint32 bits) [n_l]) as
        new CUDA tensors.  Synchronises."""
        if self.lattice is None:
            raise ValueError("targets: run first")
        n = self.lattice
        out = dict(S=torch.empty((n,), dtype=torch.int64, device=self._dev), W=torch.empty((n,), dtype=torch.int64, device=self._dev),
                   used=torch.empty((n,), dtype=torch.int32, device=self._dev))
        self.ctx.wait_torch_stream()          # the outputs are torch's allocations
        self.targets_into(**out)
        self.ctx.sync()
        return out

    def downscale(self, colour, f):
        """a colour plane (CUDA uint8 [rows, cols, 3]) at 1 / f of its resolution: the mean over f x f boxes, halves rounded up, the rest
        of the rows and columns cropped -> a new CUDA tensor [rows // f, cols // f, 3].  Asynchronous on the context's stream."""
        A.cuda_tensor("colour", colour, torch.uint8, (None, None, 3), "colour: a contiguous CUDA uint8 tensor [rows, cols, 3]", self.ctx.device)
        rows, cols = RC.image_size(colour.shape[0], colour.shape[1])
        f = A.integer_in("f", f, 1, MAX_FACTOR, f"[1, {MAX_FACTOR}]")
        if rows // f < 1 or cols // f < 1:
            raise ValueError(f"a plane of {rows} x {cols} has no box of {f} x {f}")
        out = torch.empty((rows // f, cols // f, 3), dtype=torch.uint8, device=self._dev)
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_colouralign_downscale(self._h, self.ptr(colour), rows, cols, f, self.ptr(out)))
        self._held.append(colour)
        return out


def refine_keyframes(ctx, vertices, triangles, keyframes, K, rows, cols, normals=None, scales=(4, 2, 1), rounds=4, iterations=3, fixed=(0,),
                     huber=16.0, surface_tolerance=0.02, measured_tolerance=None, min_cos=0.2, two_sided=False, z_min=0.05, z_max=20.0,
                     damping=0.0, eps=1e-7, min_pairs=6, min_views=2, stride=1, timing=None):
    """The poses of the keyframes of a run (dicts with the world pose R, t and the `colour` plane, CUDA uint8 [rows, cols, 3]) refined
    against the mesh (CUDA tensors: vertices float32 [n_v, 3], triangles [n_t, 3] of 4-byte integers, optional normals), coarse to fine:
    per scale f the colour planes are box-filtered to 1 / f of their resolution, the intrinsics scaled with them, the mesh rasterised
    once at the scale's starting poses for the occlusion test, and one `ColourAligner.run` of `rounds` x `iterations` hands its poses to
    the next scale.  The keyframes' own `depthinv` planes gate only the scale 1 and only with measured_tolerance.  -> (copies of the
    keyframe dicts with R, t replaced; the result of every scale's run as `ColourAligner.run` returns it; figures: per scale dict(scale,
    used [V, 2], cost [V, 2]: the used pairs and the cost per pair of the first and of the last system of every view)).  timing: a dict
    that receives the summed device ms of `raster`, `target`, `system` and `solve`.  It changes no geometry."""
    RS.mesh_arg(vertices, triangles, None, normals)
    kfs = RC.keyframes_arg(keyframes, measured_tolerance is not None)
    rows, cols = RC.image_size(rows, cols)
    scales = scales_arg(scales, rows, cols)
    V = views_arg(len(kfs))
    fixed = fixed_arg(fixed, V)
    rule_arg(huber, damping, eps, min_pairs, min_views, rounds, iterations, stride)
    RC.cos_arg(min_cos); RC.flag_arg("two_sided", two_sided); depth_range(z_min, z_max); intrinsics(K)
    RC.tolerance_arg("surface_tolerance", surface_tolerance)
    if measured_tolerance is not None:
        RC.tolerance_arg("measured_tolerance", measured_tolerance)
    R, t = poses(np.stack([np.asarray(k["R"], np.float64) for k in kfs]), np.stack([np.asarray(k["t"], np.float64) for k in kfs]))
    colours = RC.colour_planes_arg([k["colour"] for k in kfs], V, rows, cols, ctx.device)
    n_v = vertices.shape[0]
    results, figures = [], []
    ca = ColourAligner(ctx, max(n_v, 1), V)
    rs = None
    try:
        batch = min(RS.VIEW_CHUNK, V)         # views rasterised at a time
        rs = RS.Rasteriser(ctx, max(n_v, 1), max(triangles.shape[0], 1), rows * cols * batch)
        if timing is not None:
            rs.timing(True); ca.timing(True)
            timing.update(raster=0.0, target=0.0, system=0.0, solve=0.0)
        for f in scales:
            r_f, c_f, K_f = rows // f, cols // f, scaled_intrinsics(K, f)
            planes = colours if f == 1 else [ca.downscale(c, f) for c in colours]
            surface = torch.empty((V, r_f, c_f), dtype=torch.float32, device=ca._dev)
            ctx.wait_torch_stream()
            for a in range(0, V, batch):
                rs.render_into(vertices, triangles, R[a:a + batch], t[a:a + batch], K_f, r_f, c_f, None, None, z_min, z_max, depth=surface[a:a + batch])
                if timing is not None:
                    ctx.sync()
                    timing["raster"] += sum(rs.timing(True).values())
            measured = [k["depthinv"] for k in kfs] if f == 1 and measured_tolerance is not None else None
            res = ca.run(vertices, R, t, K_f, r_f, c_f, planes, surface=surface, depthinv=measured, normals=normals, fixed=fixed, huber=huber,
                         damping=damping, eps=eps, min_pairs=min_pairs, min_views=min_views, rounds=rounds, iterations=iterations, stride=stride,
                         z_min=z_min, z_max=z_max, surface_tolerance=surface_tolerance,
                         measured_tolerance=0.0 if measured_tolerance is None else measured_tolerance, min_cos=min_cos, two_sided=two_sided)
            if timing is not None:
                for k, ms in ca.timing(True).items():
                    timing[k] += ms
            R, t = res["R"], res["t"]
            results.append(res)
            figures.append(dict(scale=f, used=res["used"].copy(), cost=cost_per_pair(res)))
        out = []
        for v, k in enumerate(kfs):
            k = dict(k)
            k["R"], k["t"] = R[v].copy(), t[v].copy()
            out.append(k)
        return out, results, figures
    finally:
        if rs is not None:
            rs.close()
        ca.close()


def figure_lines(figures, results):
    """refine_keyframes' figures as the command-line tools print them: one line per scale"""
    lines = []
    for fig, res in zip(figures, results):
        moved = [v for v in range(len(res["status"])) if int(res["status"][v]) != FIXED]
        with np.errstate(all="ignore"):
            first = float(np.nanmean(fig["cost"][moved, 0])) if moved else float("nan")
            last = float(np.nanmean(fig["cost"][moved, 1])) if moved else float("nan")
        words = ", ".join(f"{int((res['status'] == s).sum())} {STATUS[s]}" for s in range(len(STATUS)) if (res["status"] == s).any())
        lines.append(f"colour align: scale {fig['scale']}: {int(fig['used'][:, 0].sum())} -> {int(fig['used'][:, 1].sum())} used pairs, "
                     f"cost per pair {first:.4f} -> {last:.4f} grey^2, views: {words}")
    return lines
