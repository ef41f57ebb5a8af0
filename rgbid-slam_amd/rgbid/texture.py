"""A per-triangle texture atlas for triangle meshes, baked from the keyframes that see them (binding of include/rgbid_texture.h).

Every triangle owns a right-angled patch of `patch` texels along a leg in an image, two patches to a square tile, so nothing is unwrapped.
`Texturer.add` projects every texel's point of the triangle's plane into further keyframes and gates, samples and accumulates it exactly
as `rgbid.recolour` does a vertex; `Texturer.finish` turns the sums into the atlas, byte-identical to the numpy restatement of the
contract.  `texture_mesh` is the one-shot over the keyframes of a run, and `write_obj` writes the mesh, its
texture coordinates and the atlas as OBJ, MTL and PNG."""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _args as A
from . import _lib
from . import mesh as MS
from . import raster as RS
from . import recolour as RC
from ._lib import check, ci, u64, vp
from .render import Pose, depth_range, intrinsics, poses

MIN_PATCH, MAX_PATCH = 2, 30
MAX_TRIANGLES = (1 << 31) - 1
MAX_TEXELS = 1 << 28
MAX_DIM = RS.MAX_DIM
NO_VIEW = RC.NO_VIEW
MODES = RC.MODES
SIGNATURES = {
    "rgbid_texture_layout": (u64, ci, ci, vp),
    "rgbid_texture_create": (vp, vp, u64, u64),
    "rgbid_texture_destroy": (vp,),
    "rgbid_texture_begin": (vp, u64, ci, ci, ci),
    "rgbid_texture_add": (vp, vp, vp, u64, vp, u64, ci, vp, vp, ci, ci, vp),
    "rgbid_texture_finish": (vp, vp, vp, u64, vp, vp, vp),
    "rgbid_texture_uv": (vp, vp),
    "rgbid_texture_counts": (vp, ci, ci, vp),
    "rgbid_texture_timing": (vp, ci, vp),
}
EXPORTS = list(SIGNATURES)
STAGES = ("accumulate", "resolve")
COUNTS = RC.COUNTS
OUTPUTS = ("atlas", "views_used", "best_view")


class Layout(C.Structure):
    """rgbid_texture_layout_t"""
    _fields_ = [("T", C.c_int), ("W", C.c_int), ("H", C.c_int), ("tiles", C.c_ulonglong), ("tile_rows", C.c_int), ("texels_per_triangle", C.c_int)]


def patch_arg(patch):
    """-> the patch size, texels along a leg: an integer in 2 .. 30 (ValueError otherwise)"""
    return A.integer_in("patch", patch, MIN_PATCH, MAX_PATCH, f"[{MIN_PATCH}, {MAX_PATCH}]")


def triangles_count_arg(n_triangles, max_triangles=MAX_TRIANGLES):
    """-> the number of triangles of a layout: an integer in 0 .. the capacity (ValueError otherwise)"""
    return A.integer_in("n_triangles", n_triangles, 0, max_triangles, f"[0, {max_triangles}]")


def layout(n_triangles, patch=6, tiles_x=None):
    """step 1 of the contract -> dict(T, W, H, tiles, tile_rows, tiles_x, texels_per_triangle, slots).  tiles_x: tiles in a row of the
    atlas, by default max(1, ceil(sqrt(tiles))), a square atlas (ValueError for an atlas wider or higher than 16384)"""
    n_t, n = triangles_count_arg(n_triangles), patch_arg(patch)
    tiles = (n_t + 1) // 2
    if tiles_x is None:
        tiles_x = max(1, math.isqrt(tiles))
        tiles_x += tiles_x * tiles_x < tiles
    tx = A.integer("tiles_x", tiles_x)
    if tx < 1:
        raise ValueError(f"tiles_x must be at least 1, got {tiles_x!r}")
    T = n + 2
    tile_rows = max(1, -(-tiles // tx))
    if tx * T > MAX_DIM or tile_rows * T > MAX_DIM:
        raise ValueError(f"an atlas of {tx * T} x {tile_rows * T} texels is larger than {MAX_DIM} x {MAX_DIM}")
    return dict(T=T, W=tx * T, H=tile_rows * T, tiles=tiles, tile_rows=tile_rows, tiles_x=tx, texels_per_triangle=n * (n + 1) // 2 + (n - 1),
                slots=tiles * T * T)


def host_layout(n_triangles, patch, tiles_x):
    """rgbid_texture_layout: the library's own step 1, without a device -> layout()'s dict without tiles_x and slots, or None where the
    library refuses"""
    out = Layout()
    L = _lib.bind(SIGNATURES)
    if L.rgbid_texture_layout(C.c_ulonglong(n_triangles), patch, tiles_x, C.byref(out)) != 0:
        return None
    return {k: int(getattr(out, k)) for k, _ in Layout._fields_}


def capacity_arg(max_triangles, max_texels):
    """-> the capacities of a handle: 1 .. 2^31 - 1 triangles, 1 .. 2^28 texel slots (ValueError otherwise)"""
    return (A.integer_in("max_triangles", max_triangles, 1, MAX_TRIANGLES, "[1, 2^31 - 1]"),
            A.integer_in("max_texels", max_texels, 1, MAX_TEXELS, "[1, 2^28]"))


def mesh_arg(vertices, triangles, normals=None, colours=None, n_triangles=None, max_triangles=MAX_TRIANGLES, device=None):
    """-> (vertices, triangles, normals, colours) as rgbid.raster.mesh_arg takes them, with n_triangles triangles when given (ValueError
    otherwise)"""
    RS.mesh_arg(vertices, triangles, colours, normals, RC.MAX_VERTICES, max_triangles, device)
    if n_triangles is not None and triangles.shape[0] != n_triangles:
        raise ValueError(f"triangles: {n_triangles} as at begin, got {triangles.shape[0]}")
    return vertices, triangles, normals, colours


class Texturer(_lib.CtxHandle):
    """The texturing of meshes of up to max_triangles triangles and layouts of up to max_texels slots (layout()["slots"]) on the context's
    stream: begin, any number of add, finish.  timing() gives the last add's `accumulate` and the last finish's `resolve`."""
    _destroy, _signatures, _timing, _stages = "rgbid_texture_destroy", SIGNATURES, "rgbid_texture_timing", STAGES

    def __init__(self, ctx, max_triangles, max_texels):
        self.max_triangles, self.max_texels = capacity_arg(max_triangles, max_texels)
        super().__init__(ctx)
        self.layout, self.mode, self.views, self.n_triangles, self.patch = None, None, 0, None, None
        self._held = []                       # what the stream may still read
        self._created(self.L.rgbid_texture_create(C.byref(self._h), ctx._h, C.c_ulonglong(self.max_triangles), C.c_ulonglong(self.max_texels)))

    def begin(self, n_triangles, patch=6, tiles_x=None, mode="mean"):
        """clear the state for a mesh of n_triangles triangles with layout(n_triangles, patch, tiles_x), which must fit the capacities
        -> the layout"""
        lay = layout(triangles_count_arg(n_triangles, self.max_triangles), patch, tiles_x)
        m = RC.mode_arg(mode)
        if lay["slots"] > self.max_texels:
            raise ValueError(f"the layout has {lay['slots']} texel slots, the handle {self.max_texels}")
        check(self.L.rgbid_texture_begin(self._h, C.c_ulonglong(n_triangles), patch, lay["tiles_x"], m))
        self.layout, self.mode, self.views, self.n_triangles, self.patch = lay, mode, 0, int(n_triangles), patch
        return lay

    def add(self, vertices, triangles, R, t, K, rows, cols, colours, surface=None, depthinv=None, normals=None, z_min=0.05, z_max=20.0,
            surface_tolerance=0.02, measured_tolerance=0.02, min_cos=0.2, two_sided=False):
        """V further views of the mesh (CUDA tensors: vertices float32 [n_v, 3], triangles [n_t, 3] of 4-byte integers, optional normals
        [n_v, 3]); everything else is Recolourer.add's.  The library waits once, for the count of the triangles that name no vertex;
        the tensors are held until the next finish, counts or begin."""
        if self.layout is None:
            raise ValueError("add: begin first")
        dev = self.ctx.device
        mesh_arg(vertices, triangles, normals, None, self.n_triangles, self.max_triangles, dev)
        R, t = poses(R, t)
        V = RC.views_arg(len(R), self.views)
        rows, cols = RC.image_size(rows, cols)
        k = (C.c_float * 4)(*intrinsics(K))
        colours = RC.colour_planes_arg(colours, V, rows, cols, dev)
        surface = RC.depth_planes_arg("surface", surface, V, rows, cols, dev)
        depthinv = RC.depth_planes_arg("depthinv", depthinv, V, rows, cols, dev)
        lo, hi = depth_range(z_min, z_max)
        p = RC.Params(lo, hi, RC.tolerance_arg("surface_tolerance", surface_tolerance), RC.tolerance_arg("measured_tolerance", measured_tolerance),
                      RC.cos_arg(min_cos), RC.flag_arg("two_sided", two_sided))
        ptr = lambda x: x.data_ptr() if x is not None else None
        arr = (RC.View * V)(*[RC.View(Pose((C.c_double * 9)(*R[v].reshape(9)), (C.c_double * 3)(*t[v])), ptr(colours[v]), ptr(surface[v]), ptr(depthinv[v]))
                              for v in range(V)])
        self.ctx.wait_torch_stream()          # the mesh and the planes were written on torch's stream
        check(self.L.rgbid_texture_add(self._h, self.opt_ptr(vertices), self.opt_ptr(normals), C.c_ulonglong(vertices.shape[0]), self.opt_ptr(triangles),
                                       C.c_ulonglong(triangles.shape[0]), V, arr, k, rows, cols, C.byref(p)))
        self._held += [vertices, triangles, normals, colours, surface, depthinv]
        self.views += V

    def finish_into(self, triangles=None, colours_in=None, atlas=None, views_used=None, best_view=None):
        """the raw call: the given CUDA tensors (or None) filled asynchronously on the context's stream: atlas uint8 [H, W, 3], views_used
        and best_view int32 [H, W] (uint32 bits).  colours_in: the vertices' colours uint8 [n_v, 3], with the triangles, for the texels
        no view took"""
        if self.layout is None:
            raise ValueError("finish: begin first")
        H, W, dev = self.layout["H"], self.layout["W"], self.ctx.device
        n_v = 0
        if colours_in is not None:
            A.rows3("colours", colours_in, torch.uint8, device=dev)
            n_v = colours_in.shape[0]
            if triangles is None:
                raise ValueError("colours need the triangles")
            MS.mesh_arg(triangles, n_v, RC.MAX_VERTICES, self.max_triangles, dev)
            if triangles.shape[0] != self.n_triangles:
                raise ValueError(f"triangles: {self.n_triangles} as at begin, got {triangles.shape[0]}")
        RC.output_arg("atlas", atlas, torch.uint8, (H, W, 3), dev)
        RC.output_arg("views_used", views_used, A.int4, (H, W), dev)
        RC.output_arg("best_view", best_view, A.int4, (H, W), dev)
        if best_view is not None and self.mode != "best":
            raise ValueError("best_view: only after begin(mode=\"best\")")
        ptr = self.opt_ptr
        check(self.L.rgbid_texture_finish(self._h, ptr(triangles) if colours_in is not None else None, ptr(colours_in), C.c_ulonglong(n_v), ptr(atlas),
                                          ptr(views_used), ptr(best_view)))

    def finish(self, triangles=None, colours=None):
        """the atlas from the views added so far; `colours` (CUDA uint8 [n_v, 3], with the triangles) fills the texels no view was taken
        for from the vertex colours (black without it) -> dict(atlas uint8 [H, W, 3], views_used int32 [H, W], and in mode "best"
        best_view int32 [H, W], -1 = none) as new CUDA tensors.  More views may be added afterwards.  Synchronises."""
        if self.layout is None:
            raise ValueError("finish: begin first")
        H, W = self.layout["H"], self.layout["W"]
        out = dict(atlas=torch.empty((H, W, 3), dtype=torch.uint8, device=self._dev), views_used=torch.empty((H, W), dtype=torch.int32, device=self._dev))
        if self.mode == "best":
            out["best_view"] = torch.empty((H, W), dtype=torch.int32, device=self._dev)
        self.ctx.wait_torch_stream()          # the outputs are torch's allocations
        self.finish_into(triangles, colours, out["atlas"], out["views_used"], out.get("best_view"))
        self.ctx.sync()
        self._held = []
        return out

    def uv_into(self, uv):
        """the raw call: uv, a contiguous CUDA float32 tensor [n_t, 3, 2], filled asynchronously"""
        if self.layout is None:
            raise ValueError("uv: begin first")
        A.cuda_tensor("uv", uv, torch.float32, (self.n_triangles, 3, 2), f"uv: a contiguous CUDA float32 tensor [{self.n_triangles}, 3, 2]", self.ctx.device)
        check(self.L.rgbid_texture_uv(self._h, self.ptr(uv)))

    def uv(self):
        """the texture coordinates of begin's layout -> CUDA float32 [n_t, 3, 2]: u, v per corner, origin bottom-left.  Synchronises."""
        if self.layout is None:
            raise ValueError("uv: begin first")
        uv = torch.empty((self.n_triangles, 3, 2), dtype=torch.float32, device=self._dev)
        self.ctx.wait_torch_stream()
        self.uv_into(uv)
        self.ctx.sync()
        return uv

    def counts(self, first=0, views=None):
        """the (used texel, view) pairs per class of the views first .. first + views - 1 since begin (all of them by default) -> a list
        of dict(gated, outside, hidden, unmeasured, averted, taken), which sum to n_triangles * texels_per_triangle.  Synchronises."""
        first = A.integer("first", first)
        views = self.views - first if views is None else A.integer("views", views)
        if first < 0 or views < 1 or first + views > self.views:
            raise ValueError(f"counts: views {first} .. {first + views - 1} of {self.views} added")
        out = (C.c_ulonglong * (6 * views))()
        check(self.L.rgbid_texture_counts(self._h, first, views, out))
        self._held = []
        return [dict(zip(COUNTS, (int(x) for x in out[6 * v:6 * v + 6]))) for v in range(views)]


def texture_mesh(ctx, vertices, triangles, keyframes, K, rows, cols, patch=6, normals=None, colours=None, mode="mean", surface_tolerance=0.02,
                 measured_tolerance=None, min_cos=0.2, two_sided=False, z_min=0.05, z_max=20.0, tiles_x=None, batch=RC.VIEW_CHUNK, timing=None):
    """The mesh (CUDA tensors: vertices float32 [n_v, 3], triangles [n_t, 3] of 4-byte integers, optional normals and vertex colours)
    textured from the keyframes of a run (dicts with the world pose R, t and the `colour` plane): the mesh is rasterised at `batch`
    keyframe poses at a time and a keyframe colours a texel only where the mesh's own depth at the texel's pixel footprint agrees with
    the texel's within surface_tolerance metres; with measured_tolerance also only where the keyframe's own `depthinv` agrees.  colours:
    the vertex colours that fill the texels no keyframe sees -> dict(atlas uint8 [H, W, 3], uv float32 [n_t, 3, 2], views_used int32
    [H, W], counts: per keyframe dict(gated, ..., taken), layout, texels = n_t * texels per triangle, textured: those taken by at least
    one view, fallback: the others).  timing: a dict that receives the summed device ms of `raster`, `accumulate` and `resolve`."""
    RS.mesh_arg(vertices, triangles, colours, normals)
    kfs = RC.keyframes_arg(keyframes, measured_tolerance is not None)
    RC.mode_arg(mode); RC.cos_arg(min_cos); RC.flag_arg("two_sided", two_sided); depth_range(z_min, z_max); intrinsics(K)
    RC.tolerance_arg("surface_tolerance", surface_tolerance)
    if measured_tolerance is not None:
        RC.tolerance_arg("measured_tolerance", measured_tolerance)
    rows, cols = RC.image_size(rows, cols)
    batch = min(RC.batch_arg(batch), len(kfs))
    RC.views_arg(len(kfs))
    n_v, n_t = vertices.shape[0], triangles.shape[0]
    lay = layout(n_t, patch, tiles_x)
    rs = RS.Rasteriser(ctx, max(n_v, 1), max(n_t, 1), rows * cols * batch)
    tx = None
    try:
        tx = Texturer(ctx, max(n_t, 1), max(lay["slots"], 1))
        if timing is not None:
            rs.timing(True); tx.timing(True)
            timing.update(raster=0.0, accumulate=0.0, resolve=0.0)
        tx.begin(n_t, patch, lay["tiles_x"], mode)
        depth = torch.empty((batch, rows, cols), dtype=torch.float32, device=f"cuda:{ctx.device}")
        for a in range(0, len(kfs), batch):
            part = kfs[a:a + batch]
            R, t = np.stack([np.asarray(k["R"]) for k in part]), np.stack([np.asarray(k["t"]) for k in part])
            ctx.wait_torch_stream()
            rs.render_into(vertices, triangles, R, t, K, rows, cols, None, None, z_min, z_max, depth=depth[:len(part)])
            tx.add(vertices, triangles, R, t, K, rows, cols, [k["colour"] for k in part], depth[:len(part)],
                   [k["depthinv"] for k in part] if measured_tolerance is not None else None, normals, z_min, z_max, surface_tolerance,
                   0.0 if measured_tolerance is None else measured_tolerance, min_cos, two_sided)
            if timing is not None:
                ctx.sync()
                timing["raster"] += sum(rs.timing(True).values())
                timing["accumulate"] += tx.timing(True)["accumulate"]
        out = tx.finish(triangles, colours)
        if timing is not None:
            timing["resolve"] = tx.timing(True)["resolve"]
        counts = tx.counts()
        texels = n_t * lay["texels_per_triangle"]
        textured = int((out["views_used"] != 0).sum())       # an unused texel has no view
        return dict(atlas=out["atlas"], uv=tx.uv(), views_used=out["views_used"], counts=counts, layout=lay, texels=texels, textured=textured,
                    fallback=texels - textured)
    finally:
        if tx is not None:
            tx.close()
        rs.close()


# ---- files -------------------------------------------------------------------------------------------------------------------------------
def _host(x, dtype):
    return np.ascontiguousarray((x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x))).astype(dtype, copy=False)


def obj_paths(path):
    """-> (NAME.obj, NAME.mtl, NAME.png) for a path that ends in .obj (ValueError otherwise)"""
    root, ext = os.path.splitext(os.fspath(path))
    if ext.lower() != ".obj" or not os.path.basename(root):
        raise ValueError(f"a textured mesh is written as NAME.obj, got {path!r}")
    return root + ext, root + ".mtl", root + ".png"


def write_obj(path, vertices, triangles, uv, atlas, normals=None):
    """NAME.obj with its NAME.mtl and NAME.png beside it: `v` per vertex, one `vt` per corner (uv [n_t, 3, 2]), `vn` per vertex when
    normals are given, `f a/ta[/na]` with 1-based indices; floats as %.9g, which reads back bit for bit; the atlas uint8 [H, W, 3] goes
    through rgbid.tum.write_png"""
    from . import tum
    obj, mtl, png = obj_paths(path)
    v, tri = _host(vertices, np.float32).reshape(-1, 3), _host(triangles, np.int64).reshape(-1, 3) & 0xFFFFFFFF
    uv = _host(uv, np.float32).reshape(-1, 3, 2)
    nrm = None if normals is None else _host(normals, np.float32).reshape(-1, 3)
    img = _host(atlas, np.uint8)
    if len(uv) != len(tri) or (nrm is not None and len(nrm) != len(v)) or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("write_obj: uv [n_t, 3, 2], normals [n_v, 3], atlas [H, W, 3]")
    if len(tri) and int(tri.max()) >= len(v):
        raise ValueError("write_obj: a triangle names a vertex that does not exist")
    g = lambda row: " ".join("%.9g" % float(x) for x in row)
    lines = [f"mtllib {os.path.basename(mtl)}", "usemtl atlas"]
    lines += ["v " + g(p) for p in v]
    lines += ["vt " + g(c) for c in uv.reshape(-1, 2)]
    if nrm is not None:
        lines += ["vn " + g(p) for p in nrm]
    for t, (a, b, c) in enumerate(tri.tolist()):
        ref = lambda k, i: f"{i + 1}/{3 * t + k + 1}" + (f"/{i + 1}" if nrm is not None else "")
        lines.append(f"f {ref(0, a)} {ref(1, b)} {ref(2, c)}")
    tum.write_png(png, img)
    with open(mtl, "w") as f:
        f.write(f"newmtl atlas\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {os.path.basename(png)}\n")
    with open(obj, "w") as f:
        f.write("\n".join(lines) + "\n")


def read_obj(path):
    """what write_obj wrote -> dict(vertices float32 [n_v, 3], triangles uint32 [n_t, 3], uv float32 [n_t, 3, 2], normals float32 [n_v, 3]
    or None, mtl: the material file's name, texture: the image's name from it, atlas uint8 [H, W, 3]).  ValueError for anything else."""
    from . import tum
    obj = obj_paths(path)[0]
    v, vt, vn, faces, mtl = [], [], [], [], None
    with open(obj) as f:
        for line in f:
            w = line.split()
            if not w or w[0] in ("usemtl", "#"):
                continue
            if w[0] == "mtllib":
                mtl = w[1]
            elif w[0] in ("v", "vt", "vn"):
                {"v": v, "vt": vt, "vn": vn}[w[0]].append([np.float32(x) for x in w[1:]])
            elif w[0] == "f" and len(w) == 4:
                faces.append([[int(x) for x in c.split("/")] for c in w[1:]])
            else:
                raise ValueError(f"read_obj: {line.strip()!r}")
    f = np.array(faces, np.int64).reshape(len(faces), 3, -1) if faces else np.zeros((0, 3, 2), np.int64)
    n_t = len(f)
    if mtl is None or len(vt) != 3 * n_t or (n_t and (f[:, :, 1] != np.arange(1, 3 * n_t + 1).reshape(n_t, 3)).any()):
        raise ValueError("read_obj: not a file of write_obj (one vt per corner, in order)")
    if vn and (len(vn) != len(v) or (f[:, :, 2] != f[:, :, 0]).any()):
        raise ValueError("read_obj: not a file of write_obj (one vn per vertex)")
    texture = None
    with open(os.path.join(os.path.dirname(obj), mtl)) as m:
        for line in m:
            if line.startswith("map_Kd "):
                texture = line.split(None, 1)[1].strip()
    if texture is None:
        raise ValueError("read_obj: the material names no texture")
    return dict(vertices=np.array(v, np.float32).reshape(-1, 3), triangles=(f[:, :, 0] - 1).astype(np.uint32).reshape(-1, 3),
                uv=np.array(vt, np.float32).reshape(-1, 3, 2), normals=np.array(vn, np.float32).reshape(-1, 3) if vn else None, mtl=mtl, texture=texture,
                atlas=tum.read_png(os.path.join(os.path.dirname(obj), texture)))
