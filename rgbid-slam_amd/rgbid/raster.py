"""Triangle meshes seen from camera poses, without a window (binding of include/rgbid_raster.h).

`Rasteriser.render` projects an indexed triangle mesh (what `tsdf.Volume.extract` returns after its clean-up options, or any mesh of that
form) into V pinhole cameras on the device and keeps the nearest triangle per pixel: its index, the perspective-correct depth, the
interpolated colour and camera-frame normal, byte-identical to the numpy restatement of the contract.
`mesh_agreement` rasterises the mesh at every keyframe's own pose and compares its depth with what the keyframe measured: the figure of
`render.depth_agreement` and `tsdf.surface_agreement` for the mesh the user actually gets."""
import ctypes as C

import numpy as np
import torch

from . import _args as A
from . import _lib
from . import mesh as MS
from . import render as RD
from ._lib import check, ci, f32, u64, vp
from .render import Pose, depth_range, intrinsics, outputs_arg, poses, rank_value

MAX_TRIANGLES = (1 << 31) - 1
MAX_VERTICES = 1 << 31
MAX_DIM = 16384
MAX_VIEWS = 4096
SUB = 256
VIEW_CHUNK = 16
SMALL_BOX = 16
TILE = 8
TIMED_CHUNKS = 8
EMPTY = 0xFFFFFFFF
NAN_BITS = 0x7FFFFFFF
SIGNATURES = {
    "rgbid_raster_create": (vp, vp, u64, u64, u64),
    "rgbid_raster_destroy": (vp,),
    "rgbid_raster_views": (vp, vp, u64, vp, u64, vp, vp, ci, vp, vp, ci, ci, f32, f32, vp, vp, vp, vp),
    "rgbid_raster_counts": (vp, ci, vp),
    "rgbid_raster_timing": (vp, ci, vp),
}
EXPORTS = list(SIGNATURES)
STAGES = ("project", "setup", "large", "resolve")
COUNTS = ("gated", "degenerate", "empty_box", "drawn", "fragments", "pixels")
PLANES = RD.PLANES


def capacity_arg(max_vertices, max_triangles, max_pixels):
    """-> the capacities of a handle: 1 .. 2^31 vertices, 1 .. 2^31 - 1 triangles, at least one pixel (ValueError otherwise)"""
    v, t, p = A.integer("max_vertices", max_vertices), A.integer("max_triangles", max_triangles), A.integer("max_pixels", max_pixels)
    A.in_range("max_vertices", v, 1, MAX_VERTICES, "[1, 2^31]", max_vertices)
    A.in_range("max_triangles", t, 1, MAX_TRIANGLES, "[1, 2^31 - 1]", max_triangles)
    return v, t, A.in_range("max_pixels", p, 1, 1 << 38, "[1, 2^38]", max_pixels)


def image_size(rows, cols, views=1, max_pixels=None):
    """-> (rows, cols) as the library takes them: 1 .. 16384 each, 1 .. 4096 views, and rows * cols * views <= max_pixels when given
    (ValueError otherwise)"""
    r, c = RD.image_size(rows, cols, views, max_pixels)
    if r > MAX_DIM or c > MAX_DIM:
        raise ValueError(f"rows and cols must lie in [1, {MAX_DIM}], got {rows!r} x {cols!r}")
    if views > MAX_VIEWS:
        raise ValueError(f"at most {MAX_VIEWS} views per call, got {views!r}")
    return r, c


def mesh_arg(vertices, triangles, colours=None, normals=None, max_vertices=MAX_VERTICES, max_triangles=MAX_TRIANGLES, device=None):
    """-> (vertices, triangles, colours, normals): contiguous CUDA tensors float32 [n_v, 3], 4-byte integers [n_t, 3], uint8 [n_v, 3] or
    None, float32 [n_v, 3] or None, within the capacities (ValueError otherwise)"""
    A.rows3("vertices", vertices, torch.float32, device=device)
    n_v = vertices.shape[0]
    MS.mesh_arg(triangles, n_v, max_vertices, max_triangles, device)
    if colours is not None:
        A.rows3("colours", colours, torch.uint8, n_v, device)
    if normals is not None:
        A.rows3("normals", normals, torch.float32, n_v, device)
    return vertices, triangles, colours, normals


def plane_shapes(V, rows, cols):
    return {"index": ((V, rows, cols), torch.int32), "depth": ((V, rows, cols), torch.float32), "colour": ((V, rows, cols, 3), torch.uint8),
            "normal": ((V, 3, rows, cols), torch.float32)}


class Rasteriser(_lib.CtxHandle):
    """Rasteriser for meshes of up to max_vertices vertices and max_triangles triangles and rows * cols * views <= max_pixels per call, on
    the context's stream.  timing() gives the last call's stages summed over its chunks of views (zeros for a call of more than
    TIMED_CHUNKS chunks)."""
    _destroy, _signatures, _timing, _stages = "rgbid_raster_destroy", SIGNATURES, "rgbid_raster_timing", STAGES

    def __init__(self, ctx, max_vertices, max_triangles, max_pixels):
        self.max_vertices, self.max_triangles, self.max_pixels = capacity_arg(max_vertices, max_triangles, max_pixels)
        super().__init__(ctx)
        self._views = 0
        self._created(self.L.rgbid_raster_create(C.byref(self._h), ctx._h, C.c_ulonglong(self.max_vertices), C.c_ulonglong(self.max_triangles),
                                                 C.c_ulonglong(self.max_pixels)))

    def render_into(self, vertices, triangles, R, t, K, rows, cols, colours=None, normals=None, z_min=0.05, z_max=20.0, index=None, depth=None,
                    colour=None, normal=None):
        """the raw call: checked arguments, the given CUDA planes (or None) filled asynchronously on the context's stream (the library
        waits once, for the count of the triangles that name no vertex)"""
        dev = self.ctx.device
        mesh_arg(vertices, triangles, colours, normals, self.max_vertices, self.max_triangles, dev)
        R, t = poses(R, t)
        V = len(R)
        rows, cols = image_size(rows, cols, V, self.max_pixels)
        lo, hi = depth_range(z_min, z_max)
        k = (C.c_float * 4)(*intrinsics(K))
        shapes = plane_shapes(V, rows, cols)
        given = dict(index=index, depth=depth, colour=colour, normal=normal)
        for name, x in given.items():
            if x is not None:
                A.cuda_tensor(name, x, shapes[name][1], shapes[name][0], f"{name}: a contiguous CUDA {shapes[name][1]} tensor {list(shapes[name][0])}", dev)
        if colour is not None and colours is None:
            raise ValueError("the colour plane needs the vertices' colours")
        if normal is not None and normals is None:
            raise ValueError("the normal plane needs the vertices' normals")
        arr = (Pose * V)(*[Pose((C.c_double * 9)(*R[v].reshape(9)), (C.c_double * 3)(*t[v])) for v in range(V)])
        ptr = self.opt_ptr
        self._views = 0
        check(self.L.rgbid_raster_views(self._h, ptr(vertices), C.c_ulonglong(vertices.shape[0]), ptr(triangles), C.c_ulonglong(triangles.shape[0]),
                                        ptr(colours), ptr(normals), V, arr, k, rows, cols, C.c_float(lo), C.c_float(hi), ptr(index), ptr(depth),
                                        ptr(colour), ptr(normal)))
        self._views = V

    def render(self, vertices, triangles, R, t, K, rows, cols, colours=None, normals=None, z_min=0.05, z_max=20.0, outputs=("depth", "colour")):
        """the mesh (CUDA tensors: vertices float32 [n_v, 3], triangles [n_t, 3] of 4-byte integers, optional colours uint8 [n_v, 3] and
        normals float32 [n_v, 3]) seen from the world poses R [V, 3, 3], t [V, 3] through K = fx, fy, cx, cy -> a dict of the requested
        planes as CUDA tensors with a leading view axis: index int32 [V, rows, cols] (-1 = rgbid.raster.EMPTY as two's complement: no
        triangle covers the pixel), depth float32 [V, rows, cols], colour uint8 [V, rows, cols, 3], normal float32 [V, 3, rows, cols].
        Synchronises."""
        outs = outputs_arg(outputs)
        if "colour" in outs and colours is None:
            raise ValueError("the colour plane needs the vertices' colours")
        if "normal" in outs and normals is None:
            raise ValueError("the normal plane needs the vertices' normals")
        V = len(poses(R, t)[0])
        rows, cols = image_size(rows, cols, V, self.max_pixels)
        shapes = plane_shapes(V, rows, cols)
        planes = {o: torch.empty(shapes[o][0], dtype=shapes[o][1], device=self._dev) for o in outs}
        self.ctx.wait_torch_stream()   # the mesh was written, and the planes allocated, on torch's stream
        self.render_into(vertices, triangles, R, t, K, rows, cols, colours, normals, z_min, z_max, **planes)
        self.ctx.sync()
        return planes

    def counts(self):
        """the last call's counts per view -> a list of dict(gated, degenerate, empty_box, drawn, fragments, pixels).  Synchronises."""
        if not self._views:
            raise ValueError("counts: nothing was rendered")
        out = (C.c_ulonglong * (6 * self._views))()
        check(self.L.rgbid_raster_counts(self._h, self._views, out))
        return [dict(zip(COUNTS, (int(x) for x in out[6 * v:6 * v + 6]))) for v in range(self._views)]


def render_mesh(ctx, vertices, triangles, R, t, K, rows, cols, colours=None, normals=None, z_min=0.05, z_max=20.0, outputs=("depth", "colour")):
    """one-shot Rasteriser(ctx, len(vertices), len(triangles), rows * cols * views).render(...)"""
    outputs_arg(outputs); depth_range(z_min, z_max); intrinsics(K)
    mesh_arg(vertices, triangles, colours, normals)
    V = len(poses(R, t)[0])
    rows, cols = image_size(rows, cols, V)
    rs = Rasteriser(ctx, max(vertices.shape[0], 1), max(triangles.shape[0], 1), rows * cols * V)
    try:
        return rs.render(vertices, triangles, R, t, K, rows, cols, colours, normals, z_min, z_max, outputs)
    finally:
        rs.close()


def agreement_of(depth, own_depthinv):
    """one keyframe's figures from the mesh's depth plane at its pose (torch float32 [rows, cols], NaN = empty) and the keyframe's own
    inverse depth (numpy float32 [rows, cols]) -> dict(pixels, median, p90): the pixels that are drawn and that the keyframe measured
    (iD finite and > 0, z = 1 / iD in float32), and the median and 90th percentile (nearest rank) of |z_mesh - z_keyframe| over them"""
    iD = np.asarray(own_depthinv.cpu().numpy() if isinstance(own_depthinv, torch.Tensor) else own_depthinv, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        own = np.where(np.isfinite(iD) & (iD > 0), np.float32(1) / iD, np.float32(np.nan)).astype(np.float32)
    own = torch.from_numpy(own).to(depth.device)
    both = torch.isfinite(depth) & torch.isfinite(own)
    d = torch.sort((depth[both] - own[both]).abs()).values.cpu().numpy()
    return dict(pixels=int(len(d)), median=rank_value(d, 5), p90=rank_value(d, 9))


def mesh_agreement(ctx, vertices, triangles, keyframes, K, rows, cols, z_min=0.05, z_max=20.0, batch=VIEW_CHUNK):
    """How well the mesh agrees with what each keyframe measured: the mesh is rasterised at every keyframe's pose (R, t of its dict), in
    batches of `batch` views -> per keyframe dict(pixels, median, p90) of |z_mesh - 1 / iD| (tsdf.surface_agreement's statistic, nearest
    rank) over the pixels that are drawn and that the keyframe measured (`depthinv` finite and > 0); render.agreement_summary gives the
    run's figures.  It prices min_component, simplify and smooth in metres against the keyframes.  As with the volume
    (tsdf.surface_agreement), a keyframe's own contribution cannot be excluded: the mesh was cut from voxels that are means over all
    views, this keyframe's among them, so the figure flatters a surface that few keyframes saw."""
    out = []
    if not keyframes:
        return out
    rows, cols = image_size(rows, cols)
    mesh_arg(vertices, triangles)
    batch = max(1, min(int(batch), len(keyframes)))
    rs = Rasteriser(ctx, max(vertices.shape[0], 1), max(triangles.shape[0], 1), rows * cols * batch)
    try:
        for a in range(0, len(keyframes), batch):
            kfs = keyframes[a:a + batch]
            depth = rs.render(vertices, triangles, np.stack([np.asarray(k["R"]) for k in kfs]), np.stack([np.asarray(k["t"]) for k in kfs]), K, rows,
                              cols, None, None, z_min, z_max, outputs=("depth",))["depth"]
            for j, k in enumerate(kfs):
                out.append(agreement_of(depth[j], k["depthinv"]))
    finally:
        rs.close()
    return out
