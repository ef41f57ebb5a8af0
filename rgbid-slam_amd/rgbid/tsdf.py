"""Keyframes fused into a truncated signed distance volume, and the volume's surface as a triangle mesh (binding of include/rgbid_tsdf.h).

`Volume.integrate` averages the inverse-depth planes (and colours) of keyframes, as `sequence.track_chunked(cloud=..., keyframe_depth=True,
keyframe_colour=True)` leaves them on the device, into a dense voxel volume; `Volume.extract` cuts the volume's zero crossing with marching
tetrahedra into vertices, vertex colours and index triples, byte-identical to the numpy restatement of the contract.
`fuse` is the one-shot over the keyframes of a run and `write_mesh_ply` writes what any viewer opens.  `Volume.raycast` reads the surface
back at a pose (section 20), `Volume.align` proposes the pose at which a depth frame lies on it and `align_check` holds a run's keyframes
against their own model (section 21).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _args as A
from . import _lib
from ._lib import check, ci, cu, f32, f64, u64, vp
from .consist import planes_arg
from .render import Pose, agreement_summary, depth_range, image_size, intrinsics, poses, rank_value  # noqa: F401 (agreement_summary: for callers)

MAX_VOXELS = 1 << 29
MAX_VIEWS = 65535
MAX_WEIGHT = 65535
VIEW_CHUNK = 16                         # RGBID_TSDF_VIEW_CHUNK: views one launch walks; more go in further launches, in order
VOLUME_SIGNATURES = {                   # rgbid_tsdf.h
    "rgbid_tsdf_create": (vp, vp, u64, ci, ci),
    "rgbid_tsdf_destroy": (vp,),
    "rgbid_tsdf_configure": (vp, ci, ci, ci, vp, f32, f32),
    "rgbid_tsdf_reset": (vp,),
    "rgbid_tsdf_integrate": (vp, ci, vp, vp, ci, ci, f32, f32),
    "rgbid_tsdf_get_state": (vp, vp, vp, vp),
    "rgbid_tsdf_set_state": (vp, vp, vp, vp),
    "rgbid_tsdf_extract_plan": (vp, cu, vp, vp),
    "rgbid_tsdf_extract_emit": (vp, vp, vp, vp, u64, u64),
    "rgbid_tsdf_timing": (vp, ci, vp),
}
RAYCAST_SIGNATURES = {                  # rgbid_tsdf_raycast.h
    "rgbid_tsdf_pose_wc": (vp, vp),
    "rgbid_tsdf_raycast": (vp, ci, vp, vp, ci, ci, f32, f32, f32, cu, vp, vp, vp),
    "rgbid_tsdf_raycast_timing": (vp, ci, vp),
    "rgbid_tsdf_extract_normals": (vp, vp, u64),
}
ALIGN_SIGNATURES = {                    # rgbid_tsdf_align.h
    "rgbid_tsdf_align": (vp, ci, vp, vp, ci, ci, f32, f32, cu, f32, f64, f64, cu, ci, vp, vp),
    "rgbid_tsdf_align_timing": (vp, ci, vp),
}
SIGNATURES = {**VOLUME_SIGNATURES, **RAYCAST_SIGNATURES, **ALIGN_SIGNATURES}
EXPORTS, RAYCAST_EXPORTS, ALIGN_EXPORTS = list(VOLUME_SIGNATURES), list(RAYCAST_SIGNATURES), list(ALIGN_SIGNATURES)
STAGES = ("integrate", "scan", "emit")
MAX_STEPS = 65536                       # RGBID_TSDF_MAX_STEPS: (z_max - z_min) / step at most
RAYCAST_PLANES = ("depth", "normal", "colour")
ALIGN_STAGES = ("system", "solve")
ALIGN_STATUS = ("running", "converged", "few", "singular")                                                                              # RGBID_TSDF_ALIGN_*
ALIGN_STRIDES = (1, 2, 4, 8)
ALIGN_MAX_LEVELS, ALIGN_MAX_ITERATIONS, ALIGN_TERMS = 4, 256, 28
ALIGN_LEVELS = ((4, 10), (2, 10), (1, 10))
# rgbid_tsdf_align_result: 560 bytes
ALIGN_RESULT = np.dtype([("pose", "<f8", (12,)), ("status", "<i4"), ("iterations", "<i4"), ("used", "<u4", (2,)), ("sums", "<f8", (2, ALIGN_TERMS))])


class View(C.Structure):
    """rgbid_tsdf_view: a keyframe's world pose, its inverse-depth plane and its colours (or NULL) on the device"""
    _fields_ = [("pose", Pose), ("depthinv_dev", C.c_void_p), ("colour_dev", C.c_void_p)]


def capacity_arg(max_voxels, max_views):
    """-> (max_voxels, max_views) of a handle: 8 .. 2^29 voxels and 1 .. 65 535 views per call (ValueError otherwise)"""
    n, v = A.integer("max_voxels", max_voxels), A.integer("max_views", max_views)
    return A.in_range("max_voxels", n, 8, MAX_VOXELS, "[8, 2^29]", max_voxels), A.in_range("max_views", v, 1, MAX_VIEWS, f"[1, {MAX_VIEWS}]", max_views)


def grid_arg(nx, ny, nz, origin, voxel, trunc, max_voxels=MAX_VOXELS):
    """-> (nx, ny, nz, origin, voxel, trunc) as the library takes them: dimensions >= 2 with nx ny nz <= max_voxels, origin three finite
    float32 values, voxel and trunc finite float32 values > 0 (ValueError otherwise)"""
    dims = tuple(A.integer(n, v) for n, v in zip(("nx", "ny", "nz"), (nx, ny, nz)))
    if min(dims) < 2:
        raise ValueError(f"every dimension must be at least 2, got {dims}")
    if dims[0] * dims[1] * dims[2] > max_voxels:
        raise ValueError(f"{dims[0]} x {dims[1]} x {dims[2]} voxels are more than {max_voxels}")
    try:
        o = list(origin)
    except TypeError:
        raise ValueError(f"origin: three numbers, got {origin!r}")
    if len(o) != 3:
        raise ValueError(f"origin: three numbers, got {origin!r}")
    o = [A.finite32("origin", v) for v in o]
    h, tr = A.finite32("voxel", voxel), A.finite32("trunc", trunc)
    if not (h > 0 and tr > 0):
        raise ValueError(f"voxel and trunc must be > 0, got {voxel!r}, {trunc!r}")
    return dims + (o, h, tr)


def weight_arg(min_weight):
    """-> min_weight: an integer in 1 .. 65 535 (ValueError otherwise)"""
    return A.integer_in("min_weight", min_weight, 1, MAX_WEIGHT, f"[1, {MAX_WEIGHT}]")


def component_filter_arg(min_component, largest_components):
    """-> None when both are None (no filter), else (min_triangles, largest) as mesh.filter_components takes them: min_component an
    integer in 0 .. 2^32 - 1 (None: 1), largest_components an integer >= 1 or None (ValueError otherwise)"""
    if min_component is None and largest_components is None:
        return None
    from . import mesh as MS
    return MS.min_triangles_arg(1 if min_component is None else min_component), MS.largest_arg(largest_components)


def simplify_arg(simplify):
    """-> None when simplify is None (no decimation), else the cell (c0, c1, c2) in metres as simplify.simplify_mesh takes it: a finite
    scalar > 0 or three of them (ValueError otherwise)"""
    if simplify is None:
        return None
    from . import simplify as SP
    return SP.cell_arg(simplify)


def smooth_arg(smooth):
    """-> None when smooth is None (no smoothing), else dict(iterations, lam, mu, pin_boundary) as smooth.smooth_mesh takes them: smooth an
    iteration count in 0 .. 4096 or a dict with `iterations` and any of lam (0 < lam <= 1, default 0.5), mu (-2 <= mu <= 0, default -0.53),
    pin_boundary (default False) (ValueError otherwise)"""
    if smooth is None:
        return None
    from . import smooth as SO
    kw = dict(smooth) if isinstance(smooth, dict) else dict(iterations=smooth)
    unknown = sorted(set(kw) - {"iterations", "lam", "mu", "pin_boundary"})
    if unknown or "iterations" not in kw:
        raise ValueError(f"smooth: an iteration count or a dict with iterations and any of lam, mu, pin_boundary, got {smooth!r}")
    lam, mu = SO.factors_arg(kw.get("lam", 0.5), kw.get("mu", -0.53))
    pin = kw.get("pin_boundary", False)
    if not isinstance(pin, (bool, np.bool_)):
        raise ValueError(f"smooth: pin_boundary is True or False, got {pin!r}")
    return dict(iterations=SO.iterations_arg(kw["iterations"]), lam=lam, mu=mu, pin_boundary=bool(pin))


def step_arg(step, z_min, z_max):
    """-> the ray cast's sample spacing as the float32 value the library receives: finite, > 0 and with (z_max - z_min) / step <= 65 536
    for the gate's float32 values (ValueError otherwise)"""
    lo, hi = depth_range(z_min, z_max)
    s = A.finite32("step", step)
    if not s > 0:
        raise ValueError(f"step must be > 0, got {step!r}")
    if (hi - lo) / s > MAX_STEPS:
        raise ValueError(f"step {step!r} needs more than {MAX_STEPS} samples between {z_min!r} and {z_max!r}")
    return s


def raycast_outputs_arg(outputs):
    """-> the requested planes as a tuple out of depth, normal, colour (ValueError otherwise)"""
    outs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    if not outs or any(o not in RAYCAST_PLANES for o in outs):
        raise ValueError(f"outputs: some of {RAYCAST_PLANES}, got {outputs!r}")
    return outs


def align_levels_arg(levels):
    """-> the levels as a tuple of (stride, iterations): 1 .. 4 pairs, stride out of 1, 2, 4, 8, iterations >= 1 and at most 256 in all
    (ValueError otherwise)"""
    try:
        lv = [tuple(l) for l in levels]
    except TypeError:
        raise ValueError(f"levels: pairs (stride, iterations), got {levels!r}")
    if not 1 <= len(lv) <= ALIGN_MAX_LEVELS or any(len(l) != 2 for l in lv):
        raise ValueError(f"levels: 1 .. {ALIGN_MAX_LEVELS} pairs (stride, iterations), got {levels!r}")
    lv = tuple((A.integer("stride", s), A.integer("iterations", n)) for s, n in lv)
    if any(s not in ALIGN_STRIDES for s, _ in lv):
        raise ValueError(f"a stride must be one of {ALIGN_STRIDES}, got {levels!r}")
    if any(n < 1 for _, n in lv) or sum(n for _, n in lv) > ALIGN_MAX_ITERATIONS:
        raise ValueError(f"every level needs at least 1 iteration and all together at most {ALIGN_MAX_ITERATIONS}, got {levels!r}")
    return lv


def align_params_arg(huber, damping, eps, min_pixels):
    """-> (huber, damping, eps, min_pixels) as the library takes them: huber a finite float32 > 0, damping finite and >= 0, eps finite and
    > 0, min_pixels an integer in 6 .. 2^32 - 1 (ValueError otherwise)"""
    h, d, e, n = A.finite32("huber", huber), A.finite64("damping", damping), A.finite64("eps", eps), A.integer("min_pixels", min_pixels)
    if not h > 0:
        raise ValueError(f"huber must be > 0, got {huber!r}")
    if not d >= 0:
        raise ValueError(f"damping must be >= 0, got {damping!r}")
    if not e > 0:
        raise ValueError(f"eps must be > 0, got {eps!r}")
    if not 6 <= n < 1 << 32:
        raise ValueError(f"min_pixels must be at least 6, got {min_pixels!r}")
    return h, d, e, n


def align_dict(res):
    """the records of rgbid_tsdf_align (ALIGN_RESULT [V]) -> dict(R [V, 3, 3], t [V, 3], status, iterations [V], used [V, 2],
    H [V, 2, 6, 6], b [V, 2, 6], error [V, 2]); index 0 of the pairs is the first system built, 1 the last"""
    H = np.zeros((len(res), 2, 6, 6), np.float64)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            H[:, :, i, j] = H[:, :, j, i] = res["sums"][:, :, k]
            k += 1
    return dict(R=res["pose"][:, :9].reshape(-1, 3, 3).copy(), t=res["pose"][:, 9:].copy(), status=res["status"].copy(),
                iterations=res["iterations"].copy(), used=res["used"].copy(), H=H, b=res["sums"][:, :, 21:27].copy(),
                error=res["sums"][:, :, 27].copy())


def pose_wc(R, t):
    """the twelve float32 values R00 .. R22, tx, ty, tz of R_WC | t_WC as the library forms them from one world pose"""
    p = Pose((C.c_double * 9)(*np.asarray(R, np.float64).reshape(9)), (C.c_double * 3)(*np.asarray(t, np.float64).reshape(3)))
    out = (C.c_float * 12)()
    check(_lib.bind(SIGNATURES).rgbid_tsdf_pose_wc(C.byref(p), out))
    return np.array(out[:], np.float32)


def shade(normal):
    """a camera-frame normal plane float32 [3, rows, cols] (tensor or array) -> uint8 [rows, cols]: floor(255 max(0, -n_z) + 0.5) where
    the normal is finite, 0 elsewhere.  A picture of the surface lit from the camera, not a contract."""
    n = np.asarray(normal.cpu() if isinstance(normal, torch.Tensor) else normal, np.float32)
    ok = np.isfinite(n).all(0)
    v = np.floor(255.0 * np.maximum(0.0, -np.where(ok, n[2], 0).astype(np.float64)) + 0.5)
    return np.where(ok, np.clip(v, 0, 255), 0).astype(np.uint8)


def colours_arg(colours, views, rows, cols, device=None):
    """-> the colour planes as a list of `views` entries, each None or a contiguous CUDA uint8 tensor [rows, cols, 3] (ValueError
    otherwise).  colours: None (no view has colours), a sequence of such entries or one tensor [views, rows, cols, 3]"""
    if colours is None:
        return [None] * views
    if isinstance(colours, torch.Tensor):
        colours = list(colours) if colours.dim() == 4 else [colours]
    try:
        colours = list(colours)
    except TypeError:
        raise ValueError("colours: a sequence of CUDA uint8 tensors [rows, cols, 3] or None")
    if len(colours) != views:
        raise ValueError(f"{views} views need {views} colour planes, got {len(colours)}")
    for c in colours:
        if c is not None:
            A.cuda_tensor("colours", c, torch.uint8, (rows, cols, 3), f"colours: contiguous CUDA uint8 tensors [{rows}, {cols}, 3] or None", device)
    return colours


def bounds_grid(bounds, voxel, max_voxels=MAX_VOXELS):
    """the volume that covers the box bounds = x0 y0 z0 x1 y1 z1 with voxels of `voxel` metres: -> (nx, ny, nz, origin); voxel centres on
    the box's low corner, at least 2 per axis.  ValueError for a box that is not finite or inverted, and, naming the voxel size that would
    fit, for more than max_voxels voxels"""
    try:
        b = np.asarray(bounds, np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"bounds: x0 y0 z0 x1 y1 z1, got {bounds!r}")
    h = A.finite32("voxel", voxel)
    if b.shape != (6,) or not np.isfinite(b).all() or (b[3:] < b[:3]).any():
        raise ValueError(f"bounds: six finite numbers x0 y0 z0 x1 y1 z1 with x0 <= x1, y0 <= y1, z0 <= z1, got {bounds!r}")
    if not h > 0:
        raise ValueError(f"voxel must be > 0, got {voxel!r}")
    ext = b[3:] - b[:3]
    dims = [max(int(math.ceil(e / h)) + 1, 2) for e in ext]
    if dims[0] * dims[1] * dims[2] > max_voxels:
        fit = h
        while np.prod([max(math.ceil(e / fit) + 1, 2) for e in ext]) > max_voxels:
            fit *= 1.05
        raise ValueError(f"a box of {ext[0]:.3g} x {ext[1]:.3g} x {ext[2]:.3g} m needs {dims[0]} x {dims[1]} x {dims[2]} voxels of {h:g} m, more than "
                         f"{max_voxels}: a voxel of {fit:.3g} m would fit")
    return dims[0], dims[1], dims[2], [float(np.float32(v)) for v in b[:3]]


class Volume(_lib.CtxHandle):
    """A TSDF volume of up to max_voxels voxels that takes up to max_views views per integrate call, on the context's stream."""
    _destroy, _signatures, _timing, _stages = "rgbid_tsdf_destroy", SIGNATURES, "rgbid_tsdf_timing", STAGES

    def __init__(self, ctx, max_voxels, max_views, colour=True):
        self.max_voxels, self.max_views = capacity_arg(max_voxels, max_views)
        super().__init__(ctx)
        self.colour = bool(colour)
        self.nx = self.ny = self.nz = 2
        self.origin, self.voxel, self.trunc = [0.0, 0.0, 0.0], 1.0, 1.0   # a new handle's shape (rgbid_tsdf_create)
        self._created(self.L.rgbid_tsdf_create(C.byref(self._h), ctx._h, C.c_ulonglong(self.max_voxels), self.max_views, int(self.colour)))

    @property
    def shape(self):
        return (self.nz, self.ny, self.nx)

    def _own_tensor(self, x, dtype, shape, what):
        """-> x: a contiguous CUDA tensor of `dtype` and `shape` on the volume's device (ValueError(what, and the device) otherwise)"""
        what += f" on device {self.ctx.device}"
        if A.cuda_tensor(None, x, dtype, shape, what).device.index != self.ctx.device:
            raise ValueError(what)
        return x

    def configure(self, nx, ny, nz, origin, voxel, trunc):
        """the volume's shape (nx ny nz voxels of `voxel` metres, the centre of voxel (0, 0, 0) at `origin`, truncation `trunc` metres),
        and a reset"""
        nx, ny, nz, o, h, tr = grid_arg(nx, ny, nz, origin, voxel, trunc, self.max_voxels)
        check(self.L.rgbid_tsdf_configure(self._h, nx, ny, nz, (C.c_float * 3)(*o), h, tr))
        self.nx, self.ny, self.nz, self.origin, self.voxel, self.trunc = nx, ny, nz, o, h, tr

    def reset(self):
        check(self.L.rgbid_tsdf_reset(self._h))

    def integrate(self, planes, colours, R, t, K, rows, cols, z_min=0.05, z_max=20.0):
        """fuse the views R [V, 3, 3], t [V, 3] with the inverse-depth `planes` and `colours` (None, or per view None or a CUDA uint8
        [rows, cols, 3]) into the volume, in this order.  Asynchronous on the context's stream (planes and colours written on torch's
        stream are waited for first); they must stay unchanged until it has run."""
        R, t = poses(R, t)
        V = len(R)
        rows, cols = image_size(rows, cols)
        if V > self.max_views:
            raise ValueError(f"{V} views are more than the volume's {self.max_views}")
        planes = planes_arg(planes, V, rows, cols, self.ctx.device)
        colours = colours_arg(colours, V, rows, cols, self.ctx.device)
        lo, hi = depth_range(z_min, z_max)
        k = (C.c_float * 4)(*intrinsics(K))
        views = (View * V)(*[View(Pose((C.c_double * 9)(*R[v].reshape(9)), (C.c_double * 3)(*t[v])), planes[v].data_ptr(),
                                  colours[v].data_ptr() if colours[v] is not None else None) for v in range(V)])
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_tsdf_integrate(self._h, V, views, k, rows, cols, lo, hi))

    def state(self):
        """-> (D float32 [nz, ny, nx], counts int32 [nz, ny, nx] = W | Cn << 16, rgb_sum int32 [3, nz, ny, nx]) as new CUDA tensors.
        Synchronises."""
        D = torch.empty(self.shape, dtype=torch.float32, device=self._dev)
        counts = torch.empty(self.shape, dtype=torch.int32, device=self._dev)
        rgb = torch.empty((3,) + self.shape, dtype=torch.int32, device=self._dev)
        self.ctx.wait_torch_stream()   # the outputs are torch's allocations
        check(self.L.rgbid_tsdf_get_state(self._h, D.data_ptr(), counts.data_ptr(), rgb.data_ptr()))
        self.ctx.sync()
        return D, counts, rgb

    def set_state(self, D, counts, rgb_sum=None):
        """replace the state by CUDA tensors of state()'s shapes (counts and rgb_sum int32 or uint32 bits; None: zeros).  Synchronises."""
        def plane(name, x, dtype, shape):
            if x is not None:
                return self._own_tensor(x, dtype, shape, f"{name}: a contiguous CUDA tensor {list(shape)} of 4-byte elements").data_ptr()
        d = plane("D", D, torch.float32, self.shape)
        c = plane("counts", counts, A.int4, self.shape)
        s = plane("rgb_sum", rgb_sum, A.int4, (3,) + self.shape)
        if s is not None and not self.colour:
            raise ValueError("rgb_sum: the volume holds no colour")
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_tsdf_set_state(self._h, d, c, s))
        self.ctx.sync()

    def extract(self, min_weight=1, colours=True, normals=False, min_component=None, largest_components=None, simplify=None,
                smooth=None, fill_holes=None, denoise=None, refine=None):
        """the surface among the voxels of weight >= min_weight -> (vertices float32 [nv, 3], colours uint8 [nv, 3] or None, triangles
        int32 [nt, 3] holding the uint32 vertex indices) as CUDA tensors; with normals a fourth element, the vertices' world-frame unit
        normals float32 [nv, 3] (0 0 0 where the gradient vanishes).  With min_component (triangles a connected component needs to stay)
        or largest_components (only the k largest stay) the mesh goes through mesh.filter_components and
        `last_filter` holds its figures; with both None nothing more is done.  With simplify (the cell in metres, a scalar or three
        values) the mesh, after that filter, is decimated by simplify.simplify_mesh and `last_simplify` holds its
        figures; with None nothing more is done.  With smooth (an iteration count, or a dict of iterations, lam, mu, pin_boundary) the
        vertices of the mesh, after both, are moved by smooth.smooth_mesh (Taubin's filter), the normals are
        recomputed from the smoothed triangles (area-weighted) and `last_smooth` holds its figures; with None nothing more is done.
        With fill_holes (the longest loop to close, or a dict of max_edges, any_facing) the closed loops of boundary edges of the mesh,
        after the filter and the decimation and before the smoothing, get a fan of triangles around a new vertex each
        (holes.fill_holes) and `last_fill` holds its thirteen counts; with None nothing more is done.
        With denoise (a count of normal iterations, or a dict of normal_iterations, vertex_iterations, threshold) the vertices of the
        mesh, after the filter, the decimation and the filling and before the smoothing, are moved by denoise.denoise_mesh (the filter
        that keeps sharp edges), the normals are recomputed from the denoised triangles (area-weighted) and
        `last_denoise` holds its figures; with None nothing more is done.  With refine (the longest edge to keep in metres, or a dict of
        max_edge, rounds, caps_only) the edges of the mesh above that length, after the filling and before the denoising and the
        smoothing, are split at their midpoints by refine.refine_mesh and `last_refine` holds its figures;
        caps_only needs fill_holes and splits only the fans it appended and the neighbours that share a split rim edge; with None
        nothing more is done.  Synchronises."""
        w = weight_arg(min_weight)
        component_filter = component_filter_arg(min_component, largest_components)
        cell = simplify_arg(simplify)
        fairing = smooth_arg(smooth)
        filling = None
        if fill_holes is not None:         # without the option rgbid.holes is not imported
            from . import holes as HO
            filling = HO.fill_holes_arg(fill_holes)
        denoising = None
        if denoise is not None:            # without the option rgbid.denoise is not imported
            from . import denoise as DN
            denoising = DN.denoise_arg(denoise)
        refining = None
        if refine is not None:             # without the option rgbid.refine is not imported
            from . import refine as RF
            refining = RF.refine_arg(refine)
            if refining["caps_only"] and filling is None:
                raise ValueError("refine: caps_only needs fill_holes")
        nv, nt = C.c_ulonglong(), C.c_ulonglong()
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_tsdf_extract_plan(self._h, w, C.byref(nv), C.byref(nt)))
        verts = torch.empty((nv.value, 3), dtype=torch.float32, device=self._dev)
        cols = torch.empty((nv.value, 3), dtype=torch.uint8, device=self._dev) if colours else None
        tris = torch.empty((nt.value, 3), dtype=torch.int32, device=self._dev)
        nrm = torch.empty((nv.value, 3), dtype=torch.float32, device=self._dev) if normals else None
        self.ctx.wait_torch_stream()   # the outputs are torch's allocations
        self.emit(verts, cols, tris)
        if normals:
            self.emit_normals(nrm)
        self.ctx.sync()
        if component_filter is not None:
            from . import mesh as MS
            verts, cols, tris, nrm, self.last_filter = MS.filter_components(self.ctx, verts, cols, tris, nrm, *component_filter)
        if cell is not None:
            from . import simplify as SP
            verts, cols, tris, nrm, self.last_simplify = SP.simplify_mesh(self.ctx, verts, cols, tris, nrm, cell=cell)
        if filling is not None:
            n_before = tris.shape[0]
            verts, cols, tris, nrm, self.last_fill = HO.fill_holes(self.ctx, verts, cols, tris, nrm, **filling)
        if refining is not None:
            caps = RF.cap_selection(n_before, tris.shape[0], self._dev) if refining["caps_only"] else None
            verts, cols, tris, nrm, _, self.last_refine = RF.refine_mesh(self.ctx, verts, cols, tris, nrm, refining["max_edge"], refining["rounds"], caps)
        if denoising is not None:
            verts, nrm, self.last_denoise = DN.denoise_mesh(self.ctx, verts, tris, normals=normals and fairing is None, **denoising)
        if fairing is not None:
            from . import smooth as SO
            verts, nrm, self.last_smooth = SO.smooth_mesh(self.ctx, verts, tris, normals=normals, **fairing)
        return (verts, cols, tris, nrm) if normals else (verts, cols, tris)

    def emit_normals(self, normals):
        """write the last plan's vertex normals into a CUDA tensor [>= nv, 3] float32.  Asynchronous."""
        assert normals.is_cuda and normals.dtype == torch.float32 and normals.is_contiguous() and normals.dim() == 2 and normals.shape[1] == 3
        check(self.L.rgbid_tsdf_extract_normals(self._h, self.ptr(normals), C.c_ulonglong(normals.shape[0])))

    def _raycast_args(self, R, t, K, rows, cols, step, min_weight, z_min, z_max):
        """the ray cast's arguments as the library takes them (ValueError for what it would refuse)"""
        R, t = poses(R, t)
        rows, cols = image_size(rows, cols, len(R), (1 << 31) - 1)
        if len(R) > self.max_views:
            raise ValueError(f"{len(R)} views are more than the volume's {self.max_views}")
        lo, hi = depth_range(z_min, z_max)
        return R, t, intrinsics(K), rows, cols, step_arg(self.voxel if step is None else step, lo, hi), weight_arg(min_weight), lo, hi

    def raycast_into(self, R, t, K, rows, cols, step, min_weight, z_min, z_max, depth=None, normal=None, colour=None):
        """the raw call: checked arguments, the given CUDA planes (or None) filled asynchronously on the context's stream: depth float32
        [V, rows, cols], normal float32 [V, 3, rows, cols], colour uint8 [V, rows, cols, 3], contiguous"""
        R, t, k, rows, cols, s, w, lo, hi = self._raycast_args(R, t, K, rows, cols, step, min_weight, z_min, z_max)
        V = len(R)
        k = (C.c_float * 4)(*k)
        shapes = dict(depth=((V, rows, cols), torch.float32), normal=((V, 3, rows, cols), torch.float32), colour=((V, rows, cols, 3), torch.uint8))
        for name, x in (("depth", depth), ("normal", normal), ("colour", colour)):
            if x is not None:
                self._own_tensor(x, shapes[name][1], shapes[name][0], f"{name}: a contiguous CUDA {shapes[name][1]} tensor {list(shapes[name][0])}")
        arr = (Pose * V)(*[Pose((C.c_double * 9)(*R[v].reshape(9)), (C.c_double * 3)(*t[v])) for v in range(V)])
        ptr = self.opt_ptr
        check(self.L.rgbid_tsdf_raycast(self._h, V, arr, k, rows, cols, C.c_float(lo), C.c_float(hi), C.c_float(s), w, ptr(depth), ptr(normal),
                                        ptr(colour)))

    def raycast(self, R, t, K, rows, cols, step=None, min_weight=1, z_min=0.05, z_max=20.0, outputs=RAYCAST_PLANES):
        """the fused surface seen from the world poses R [V, 3, 3], t [V, 3] through K = fx, fy, cx, cy: every pixel's ray is marched
        through the volume in samples `step` metres of camera depth apart (None: the voxel size) up to the first crossing from positive
        to negative D among voxels of weight >= min_weight -> a dict of the requested planes as CUDA tensors: depth float32
        [V, rows, cols] (NaN: no surface), normal float32 [V, 3, rows, cols] in the camera frame, colour uint8 [V, rows, cols, 3].
        A step above trunc / |ray direction| may step over the band.  Synchronises."""
        outs = raycast_outputs_arg(outputs)
        R, t, _, rows, cols, step, min_weight, z_min, z_max = self._raycast_args(R, t, K, rows, cols, step, min_weight, z_min, z_max)
        V = len(R)
        shape = {"depth": ((V, rows, cols), torch.float32), "normal": ((V, 3, rows, cols), torch.float32), "colour": ((V, rows, cols, 3), torch.uint8)}
        planes = {o: torch.empty(shape[o][0], dtype=shape[o][1], device=self._dev) for o in outs}
        self.ctx.wait_torch_stream()   # the outputs are torch's allocations
        self.raycast_into(R, t, K, rows, cols, step, min_weight, z_min, z_max, **planes)
        self.ctx.sync()
        return planes

    def raycast_timing(self, enable=True):
        """record HIP events around the following ray casts (the switch is `timing`'s); -> the device ms of the last one"""
        return self._stage_ms("rgbid_tsdf_raycast_timing", ("raycast",), int(enable))["raycast"]

    def _align_args(self, R, t, K, rows, cols, levels, huber, damping, eps, min_pixels, min_weight, z_min, z_max):
        """the alignment's arguments as the library takes them (ValueError for what it would refuse)"""
        R, t = poses(R, t)
        rows, cols = image_size(rows, cols, len(R), (1 << 31) - 1)
        if len(R) > self.max_views:
            raise ValueError(f"{len(R)} views are more than the volume's {self.max_views}")
        lo, hi = depth_range(z_min, z_max)
        h, d, e, n = align_params_arg(self.trunc if huber is None else huber, damping, eps, min_pixels)
        return R, t, intrinsics(K), rows, cols, align_levels_arg(levels), h, d, e, n, weight_arg(min_weight), lo, hi

    def align_into(self, planes, R, t, K, rows, cols, levels, huber, damping, eps, min_pixels, min_weight, z_min, z_max, result):
        """the raw call: checked arguments, the records written asynchronously on the context's stream into `result`, a contiguous CUDA
        uint8 tensor of 560 bytes per view"""
        R, t, k, rows, cols, lv, h, d, e, n, w, lo, hi = self._align_args(R, t, K, rows, cols, levels, huber, damping, eps, min_pixels, min_weight,
                                                                           z_min, z_max)
        V = len(R)
        planes = planes_arg(planes, V, rows, cols, self.ctx.device)
        if not (isinstance(result, torch.Tensor) and result.is_cuda and result.dtype == torch.uint8 and result.is_contiguous()
                and result.numel() == V * ALIGN_RESULT.itemsize and result.device.index == self.ctx.device and result.data_ptr() % 8 == 0):
            raise ValueError(f"result: a contiguous CUDA uint8 tensor of {V} x {ALIGN_RESULT.itemsize} bytes on device {self.ctx.device}")
        views = (View * V)(*[View(Pose((C.c_double * 9)(*R[v].reshape(9)), (C.c_double * 3)(*t[v])), planes[v].data_ptr(), None) for v in range(V)])
        lv_arr = (C.c_int * (2 * len(lv)))(*[x for l in lv for x in l])
        check(self.L.rgbid_tsdf_align(self._h, V, views, (C.c_float * 4)(*k), rows, cols, C.c_float(lo), C.c_float(hi), w, C.c_float(h),
                                      C.c_double(d), C.c_double(e), n, len(lv), lv_arr, C.c_void_p(result.data_ptr())))

    def align(self, planes, R, t, K, rows, cols, levels=ALIGN_LEVELS, huber=None, damping=0.0, eps=1e-6, min_pixels=64, min_weight=1,
              z_min=0.05, z_max=20.0):
        """propose, for each view, the world pose at which its inverse-depth plane lies on the volume's surface: Gauss-Newton on the
        interpolated signed distance of every measured pixel, from the poses R [V, 3, 3], t [V, 3], over the `levels` (stride,
        iterations) in order, with the Huber threshold `huber` in metres (None: trunc), the damping H_jj (1 + damping), the step bound
        `eps` that ends a level, and at least `min_pixels` used pixels -> dict(R [V, 3, 3], t [V, 3] float64, status [V] (an index into
        ALIGN_STATUS), iterations [V], used [V, 2], H [V, 2, 6, 6], b [V, 2, 6], error [V, 2]: the normal equations H delta = -b for
        delta = (v, omega) in the world frame and the weighted squared residual, of the first and of the last system built).  Nothing is
        applied: the caller judges the proposal.  Synchronises."""
        a = self._align_args(R, t, K, rows, cols, levels, huber, damping, eps, min_pixels, min_weight, z_min, z_max)
        V = len(a[0])
        planes_arg(planes, V, a[3], a[4], self.ctx.device)
        result = torch.empty((V * ALIGN_RESULT.itemsize,), dtype=torch.uint8, device=self._dev)
        self.ctx.wait_torch_stream()   # the planes and the result are torch's
        self.align_into(planes, R, t, K, rows, cols, levels, huber, damping, eps, min_pixels, min_weight, z_min, z_max, result)
        self.ctx.sync()
        return align_dict(result.cpu().numpy().view(ALIGN_RESULT))

    def align_timing(self, enable=True):
        """record HIP events around every launch of the following alignments (the switch is `timing`'s); -> the device ms of the last
        call, summed over its launches {stage: ms}"""
        return self._stage_ms("rgbid_tsdf_align_timing", ALIGN_STAGES, int(enable))

    def emit(self, vertices, colours, triangles):
        """write the last plan's mesh into CUDA tensors [>= nv, 3] float32, [>= nv, 3] uint8 or None, [>= nt, 3] int32.  Asynchronous."""
        assert vertices.is_cuda and vertices.dtype == torch.float32 and vertices.is_contiguous() and vertices.dim() == 2 and vertices.shape[1] == 3
        assert triangles.is_cuda and triangles.element_size() == 4 and triangles.is_contiguous() and triangles.dim() == 2 and triangles.shape[1] == 3
        if colours is not None:
            assert colours.is_cuda and colours.dtype == torch.uint8 and colours.is_contiguous() and tuple(colours.shape) == tuple(vertices.shape)
        ptr = self.opt_ptr
        check(self.L.rgbid_tsdf_extract_emit(self._h, ptr(vertices), ptr(colours), ptr(triangles), C.c_ulonglong(vertices.shape[0]),
                                             C.c_ulonglong(triangles.shape[0])))

def cloud_bounds(points, pad=0.0):
    """the bounding box x0 y0 z0 x1 y1 z1 of the finite records of a cloud (CUDA uint8 [M, 32]), padded by `pad` metres; None without one"""
    xyz = points.view(torch.float32)[:, :3]
    xyz = xyz[torch.isfinite(xyz).all(1)]
    if not len(xyz):
        return None
    lo, hi = xyz.min(0).values.cpu().numpy().astype(np.float64), xyz.max(0).values.cpu().numpy().astype(np.float64)
    return [float(v) for v in np.concatenate([lo - pad, hi + pad])]


def fuse(ctx, keyframes, K, rows, cols, bounds=None, voxel=0.02, trunc=None, min_weight=1, z_min=0.05, z_max=20.0, max_voxels=1 << 27,
         points=None, return_volume=False, normals=False, keep_volume=False, min_component=None, largest_components=None, simplify=None,
         smooth=None, recolour=None, recolour_tolerance=None, recolour_measured=None, fill_holes=None, colour_align=None,
         denoise=None, refine=None):
    """one-shot over the keyframes of a run (ChunkCloud.keyframes with `depthinv` and, for a coloured mesh, `colour`): a volume over
    `bounds` = x0 y0 z0 x1 y1 z1 (None: the box of the cloud `points`, padded by trunc) with voxels of `voxel` metres, every keyframe
    integrated in order with its world pose, the surface extracted -> (vertices, colours, triangles) as CUDA tensors, with normals
    also the vertex normals, with return_volume also a dict of the volume's figures (nx, ny, nz, origin, voxels, touched), with
    keep_volume also the open Volume, which the caller closes (in this order).  trunc defaults to 4 voxel.  min_component and
    largest_components are Volume.extract's: with one of them the mesh loses its small connected components and the volume's figures
    gain `filter`, the components, vertices and triangles before and after.  simplify is Volume.extract's too: the mesh is decimated by
    vertex clustering with that cell and the volume's figures gain `simplify`.  smooth is Volume.extract's as well: the vertices are moved
    by Taubin's filter last, the normals are those of the smoothed surface and the volume's figures gain `smooth`.  fill_holes is Volume.extract's:
    the small holes are closed before the smoothing and the volume's figures gain `fill_holes`, the thirteen counts.  denoise is
    Volume.extract's: the vertices are moved by the filter that keeps sharp edges after the filling and before the smoothing, the normals
    are those of the denoised surface and the volume's figures gain `denoise`.  refine is Volume.extract's: the edges above a length are
    split after the filling and before the denoising and the volume's figures gain `refine`.  recolour = "mean" or
    "best" replaces the colours of the mesh that is returned, after every other option, by what the keyframes show at full resolution
    (rgbid.recolour.recolour_mesh, DESIGN.md section 27: every keyframe needs its `colour`): a keyframe colours a vertex where the mesh's
    own depth at its pose agrees with the vertex's within recolour_tolerance metres (None: 2 voxel) and, with recolour_measured, where
    its own `depthinv` agrees within that many metres; the mesh's normals weight the keyframes when it has them; a vertex no keyframe
    sees keeps its colour; the volume's figures gain `recolour`: the vertices, those a keyframe coloured, the (vertex, keyframe) pairs
    per class.  None leaves every byte as it is.  colour_align (a dict of rgbid.colouralign.refine_keyframes' keywords, possibly empty)
    refines the keyframes' poses against the colours of the mesh that is returned before recolour samples them (DESIGN.md section 31;
    surface_tolerance defaults to recolour's); the volume's figures gain `colour_align`: the refined keyframes, every scale's result
    and figures.  The volume and the mesh's geometry are those of the given poses.  None leaves every byte as it is."""
    trunc = 4.0 * voxel if trunc is None else trunc
    if colour_align is not None:
        from . import colouralign as CA  # colouralign imports raster and recolour, which need nothing of this module
        colour_align = dict(colour_align)
        CA.RC.keyframes_arg(keyframes, colour_align.get("measured_tolerance") is not None)
        CA.scales_arg(colour_align.get("scales", (4, 2, 1)), rows, cols)
        colour_align.setdefault("surface_tolerance", 2.0 * voxel if recolour_tolerance is None else recolour_tolerance)
    if recolour is not None:
        from . import recolour as RC     # recolour imports raster, which needs nothing of this module
        RC.mode_arg(recolour)
        RC.keyframes_arg(keyframes, recolour_measured is not None)
        recolour_tolerance = RC.tolerance_arg("recolour_tolerance", 2.0 * voxel if recolour_tolerance is None else recolour_tolerance)
        if recolour_measured is not None:
            RC.tolerance_arg("recolour_measured", recolour_measured)
    elif recolour_tolerance is not None or recolour_measured is not None:
        raise ValueError("recolour_tolerance and recolour_measured need recolour")
    w = weight_arg(min_weight)
    component_filter_arg(min_component, largest_components)
    simplify_arg(simplify)
    smooth_arg(smooth)
    if fill_holes is not None:
        from . import holes as HO
        HO.fill_holes_arg(fill_holes)
    if denoise is not None:
        from . import denoise as DN
        DN.denoise_arg(denoise)
    if refine is not None:
        from . import refine as RF
        if RF.refine_arg(refine)["caps_only"] and fill_holes is None:
            raise ValueError("refine: caps_only needs fill_holes")
    if not keyframes:
        raise ValueError("no keyframes to fuse")
    if bounds is None:
        bounds = cloud_bounds(points, A.finite32("trunc", trunc)) if points is not None else None
        if bounds is None:
            raise ValueError("bounds: needed without a cloud of finite points")
    nx, ny, nz, origin = bounds_grid(bounds, voxel, max_voxels)
    grid_arg(nx, ny, nz, origin, voxel, trunc)
    has_colour = all(kf.get("colour") is not None for kf in keyframes)
    V = len(keyframes)
    vol = Volume(ctx, nx * ny * nz, min(V, MAX_VIEWS), colour=has_colour)
    try:
        vol.configure(nx, ny, nz, origin, voxel, trunc)
        for a in range(0, V, MAX_VIEWS):
            kfs = keyframes[a:a + MAX_VIEWS]
            vol.integrate([k["depthinv"] for k in kfs], [k["colour"] for k in kfs] if has_colour else None, np.stack([k["R"] for k in kfs]),
                          np.stack([k["t"] for k in kfs]), K, rows, cols, z_min, z_max)
        filtered = min_component is not None or largest_components is not None
        mesh = vol.extract(w, colours=True, normals=normals, min_component=min_component, largest_components=largest_components, simplify=simplify,
                           smooth=smooth, fill_holes=fill_holes, denoise=denoise, refine=refine)
        if colour_align is not None:
            refined, results, figures = CA.refine_keyframes(ctx, mesh[0], mesh[2], keyframes, K, rows, cols, mesh[3] if normals else None,
                                                            z_min=z_min, z_max=z_max, **colour_align)
            aligned = dict(keyframes=refined, results=results, figures=figures)
            keyframes = refined               # what recolour samples; the volume was integrated above
        if recolour is not None:
            nrm = mesh[3] if normals else None
            new_colours, used, pairs = RC.recolour_mesh(ctx, mesh[0], mesh[2], keyframes, K, rows, cols, nrm, mesh[1], recolour, recolour_tolerance,
                                                        recolour_measured, z_min=z_min, z_max=z_max)
            mesh = (mesh[0], new_colours) + tuple(mesh[2:])
            recoloured = dict(mode=recolour, vertices=int(used.shape[0]), coloured=int((used != 0).sum().item()), **RC.counts_total(pairs))
        if return_volume:
            _, counts, _ = vol.state()
            mesh += (dict(nx=nx, ny=ny, nz=nz, origin=origin, voxels=nx * ny * nz, touched=int(((counts & 0xFFFF) != 0).sum().item())),)
            if filtered:
                mesh[-1]["filter"] = vol.last_filter
            if simplify is not None:
                mesh[-1]["simplify"] = vol.last_simplify
            if fill_holes is not None:
                mesh[-1]["fill_holes"] = vol.last_fill
            if refine is not None:
                mesh[-1]["refine"] = vol.last_refine
            if denoise is not None:
                mesh[-1]["denoise"] = vol.last_denoise
            if smooth is not None:
                mesh[-1]["smooth"] = vol.last_smooth
            if recolour is not None:
                mesh[-1]["recolour"] = recoloured
            if colour_align is not None:
                mesh[-1]["colour_align"] = aligned
        if keep_volume:
            mesh += (vol,)
            vol = None
        return mesh
    finally:
        if vol is not None:
            vol.close()


def surface_agreement(vol, keyframes, K, rows, cols, step=None, min_weight=1, z_min=0.05, z_max=20.0):
    """How well the fused surface agrees with what each keyframe measured: the volume is ray-cast at every keyframe's pose (R, t of its
    dict), in batches of at most the handle's views -> per keyframe dict(pixels, median, p90) of |z_cast - 1 / iD| (nearest rank) over the
    pixels that hit and that the keyframe measured (`depthinv` finite and > 0); render.agreement_summary gives the run's figures.
    Unlike render.depth_agreement, which ignores a keyframe's own records, a keyframe's own contribution to the volume cannot be
    excluded: every voxel is a mean over all views, so the figure flatters a surface that few keyframes saw."""
    out = []
    for a in range(0, len(keyframes), vol.max_views):
        kfs = keyframes[a:a + vol.max_views]
        depth = vol.raycast(np.stack([np.asarray(k["R"]) for k in kfs]), np.stack([np.asarray(k["t"]) for k in kfs]), K, rows, cols, step,
                            min_weight, z_min, z_max, outputs=("depth",))["depth"]
        for j, k in enumerate(kfs):
            iD = k["depthinv"]
            iD = np.asarray(iD.cpu().numpy() if isinstance(iD, torch.Tensor) else iD, np.float32)
            with np.errstate(divide="ignore", invalid="ignore"):
                own = np.where(np.isfinite(iD) & (iD > 0), np.float32(1) / iD, np.float32(np.nan)).astype(np.float32)
            own = torch.from_numpy(own).to(depth.device)
            both = torch.isfinite(depth[j]) & torch.isfinite(own)
            d = torch.sort((depth[j][both] - own[both]).abs()).values.cpu().numpy()
            out.append(dict(pixels=int(len(d)), median=rank_value(d, 5), p90=rank_value(d, 9)))
    return out


def pose_correction(R0, t0, R1, t1):
    """the rotation angle (rad) and the translation (m) that take the world pose (R0, t0) to (R1, t1)"""
    dR = np.asarray(R1, np.float64) @ np.asarray(R0, np.float64).T
    c = min(1.0, max(-1.0, (float(np.trace(dR)) - 1.0) / 2.0))
    return math.acos(c), float(np.linalg.norm(np.asarray(t1, np.float64) - np.asarray(t0, np.float64)))


def align_check(ctx, keyframes, K, rows, cols, bounds=None, voxel=0.02, trunc=None, levels=ALIGN_LEVELS, huber=None, damping=0.0, eps=1e-6,
                min_pixels=64, min_weight=1, z_min=0.05, z_max=20.0, max_voxels=1 << 27, points=None, return_results=False):
    """A consistency check of a run's keyframe poses against its own model: the even-numbered keyframes are fused (as `fuse` does, over
    `bounds` or the box of `points`), every odd-numbered one is aligned to that model from its own pose -> per odd keyframe
    dict(keyframe, rotation (rad), translation (m): the correction the alignment proposes, status (a word of ALIGN_STATUS), iterations,
    used, rms_before, rms_after: sqrt(error / used) of the first and the last system, NaN without a used pixel); with return_results also
    Volume.align's dict.  Nothing is applied.  A CPU prototype showed why: when a volume is fused from perturbed views and every view
    is aligned to it and fused again, the poses get worse round by round, and tracking then integrating view by view doubled the
    rotation error -- the surfaces here are near-planar, the model is thin and aligning a view to a model it is part of is biased.  The
    corrections are a diagnostic of the trajectory, not a refinement of it."""
    even, odd = keyframes[0::2], keyframes[1::2]
    if not even or not odd:
        raise ValueError("the check needs at least two keyframes")
    mesh = fuse(ctx, even, K, rows, cols, bounds=bounds, voxel=voxel, trunc=trunc, min_weight=min_weight, z_min=z_min, z_max=z_max,
                max_voxels=max_voxels, points=points, keep_volume=True)
    vol = mesh[-1]
    try:
        out, results = [], []
        for a in range(0, len(odd), vol.max_views):
            kfs = odd[a:a + vol.max_views]
            r = vol.align([k["depthinv"] for k in kfs], np.stack([np.asarray(k["R"]) for k in kfs]), np.stack([np.asarray(k["t"]) for k in kfs]), K,
                          rows, cols, levels, huber, damping, eps, min_pixels, min_weight, z_min, z_max)
            results.append(r)
            for j, k in enumerate(kfs):
                rot, tr = pose_correction(k["R"], k["t"], r["R"][j], r["t"][j])
                with np.errstate(all="ignore"):
                    rms = np.sqrt(r["error"][j] / r["used"][j].astype(np.float64))
                out.append(dict(keyframe=2 * (a + j) + 1, rotation=rot, translation=tr, status=ALIGN_STATUS[int(r["status"][j])],
                                iterations=int(r["iterations"][j]), used=int(r["used"][j][1]), rms_before=float(rms[0]), rms_after=float(rms[1])))
        if return_results:
            return out, {k: np.concatenate([r[k] for r in results]) for k in results[0]}
        return out
    finally:
        vol.close()


def align_check_summary(figures):
    """align_check's figures -> dict(views, median and largest rotation and translation, counts per status word)"""
    rot, tr = [f["rotation"] for f in figures], [f["translation"] for f in figures]
    return dict(views=len(figures), rotation_median=float(np.median(rot)), rotation_max=float(max(rot)), translation_median=float(np.median(tr)),
                translation_max=float(max(tr)), status={w: sum(f["status"] == w for f in figures) for w in ALIGN_STATUS})


def _vertex_dtype(normals):
    nrm = [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")] if normals else []
    return np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + nrm + [("red", "u1"), ("green", "u1"), ("blue", "u1")])


def mesh_ply_bytes(vertices, colours, triangles, normals=None):
    """binary little-endian PLY of a mesh: element vertex with x y z (float), with normals also nx ny nz (float), and red green blue
    (uchar), element face with `property list uchar uint vertex_indices`; colours None: black.  Tensors (host or device) or numpy
    arrays."""
    host = lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    v = np.ascontiguousarray(host(vertices), "<f4").reshape(-1, 3)
    t = np.ascontiguousarray(host(triangles)).reshape(-1, 3)
    t = t.view(np.uint32) if t.dtype == np.int32 else t.astype(np.uint32)
    c = np.zeros((len(v), 3), np.uint8) if colours is None else np.ascontiguousarray(host(colours), np.uint8).reshape(-1, 3)
    assert len(c) == len(v) and (not len(t) or int(t.max()) < len(v))
    head = ("ply\nformat binary_little_endian 1.0\ncomment rgbid fused keyframe mesh\n"
            f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
            + ("property float nx\nproperty float ny\nproperty float nz\n" if normals is not None else "") +
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            f"element face {len(t)}\nproperty list uchar uint vertex_indices\nend_header\n")
    vr = np.empty(len(v), _vertex_dtype(normals is not None))
    vr["x"], vr["y"], vr["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        n = np.ascontiguousarray(host(normals), "<f4").reshape(-1, 3)
        assert len(n) == len(v)
        vr["nx"], vr["ny"], vr["nz"] = n[:, 0], n[:, 1], n[:, 2]
    vr["red"], vr["green"], vr["blue"] = c[:, 0], c[:, 1], c[:, 2]
    fr = np.empty(len(t), np.dtype([("n", "u1"), ("i", "<u4", (3,))]))
    fr["n"] = 3
    fr["i"] = t
    return head.encode("ascii") + vr.tobytes() + fr.tobytes()


def write_mesh_ply(path, vertices, colours, triangles, normals=None):
    with open(path, "wb") as f:
        f.write(mesh_ply_bytes(vertices, colours, triangles, normals))


def read_mesh_ply(data):
    """what mesh_ply_bytes wrote -> (vertices float32 [nv, 3], colours uint8 [nv, 3], triangles uint32 [nt, 3]), and as a fourth
    element the normals float32 [nv, 3] when the file holds them"""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    nv = int([l for l in head if l.startswith("element vertex")][0].split()[2])
    nt = int([l for l in head if l.startswith("element face")][0].split()[2])
    has_normals = "property float nx" in head
    vd = _vertex_dtype(has_normals)
    fd = np.dtype([("n", "u1"), ("i", "<u4", (3,))])
    assert len(data) == end + nv * vd.itemsize + nt * fd.itemsize
    v = np.frombuffer(data, vd, nv, end)
    f = np.frombuffer(data, fd, nt, end + nv * vd.itemsize)
    assert (f["n"] == 3).all()
    mesh = (np.stack([v["x"], v["y"], v["z"]], 1), np.stack([v["red"], v["green"], v["blue"]], 1), f["i"].copy())
    return mesh + (np.stack([v["nx"], v["ny"], v["nz"]], 1),) if has_normals else mesh
