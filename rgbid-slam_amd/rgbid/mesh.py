"""Connected components of an indexed triangle mesh on the device, and the mesh without its small ones (binding of include/rgbid_mesh.h).

`Components.label` finds which triangles hang together (two vertices are adjacent iff one triangle names both), `Components.select` keeps
the components of at least `min_triangles` triangles and, with a mask, only the marked ones, `Components.emit` writes the kept vertices,
their attributes and the renumbered triangles; all byte-identical to the numpy restatement of the contract.
`largest_mask` marks the k largest components of a table and `filter_components` is the one-shot that `tsdf.Volume.extract` and `tsdf.fuse`
call for their `min_component` / `largest_components` keywords."""
import ctypes as C

import numpy as np
import torch

from . import _args as A
from . import _lib
from ._lib import check, ci, cu, u64, vp

MAX_VERTICES = 1 << 31
MAX_TRIANGLES = 1 << 31
SIGNATURES = {
    "rgbid_mesh_create": (vp, vp, u64, u64),
    "rgbid_mesh_destroy": (vp,),
    "rgbid_mesh_label": (vp, u64, u64, vp, vp),
    "rgbid_mesh_components": (vp, vp, vp),
    "rgbid_mesh_select": (vp, cu, vp, vp, vp, vp),
    "rgbid_mesh_emit": (vp, vp, vp, vp, vp, vp, vp, vp, vp, u64, u64),
    "rgbid_mesh_timing": (vp, ci, vp),
}
EXPORTS = list(SIGNATURES)
STAGES = ("label", "select", "emit")


def capacity_arg(max_vertices, max_triangles):
    """-> (max_vertices, max_triangles) of a handle: each 1 .. 2^31 (ValueError otherwise)"""
    v, t = A.integer("max_vertices", max_vertices), A.integer("max_triangles", max_triangles)
    A.in_range("max_vertices", v, 1, MAX_VERTICES, "[1, 2^31]", max_vertices)
    return v, A.in_range("max_triangles", t, 1, MAX_TRIANGLES, "[1, 2^31]", max_triangles)


def mesh_arg(triangles, n_vertices, max_vertices=MAX_VERTICES, max_triangles=MAX_TRIANGLES, device=None):
    """-> (triangles, n_vertices): a contiguous CUDA tensor [n_t, 3] of 4-byte integers (int32 holding the uint32 indices, as Volume.extract
    returns them) with n_t <= max_triangles, and 0 <= n_vertices <= max_vertices, not 0 when there are triangles (ValueError otherwise)"""
    n_v = A.integer("n_vertices", n_vertices)
    A.rows3("triangles", triangles, A.int4, device=device)
    A.in_range("n_vertices", n_v, 0, max_vertices, f"[0, {max_vertices}]", n_vertices)
    if triangles.shape[0] > max_triangles:
        raise ValueError(f"{triangles.shape[0]} triangles are more than {max_triangles}")
    if triangles.shape[0] and n_v == 0:
        raise ValueError("triangles without vertices")
    return triangles, n_v


def min_triangles_arg(min_triangles):
    """-> min_triangles: an integer in 0 .. 2^32 - 1 (ValueError otherwise)"""
    return A.integer_in("min_triangles", min_triangles, 0, (1 << 32) - 1, "[0, 2^32 - 1]")


def largest_arg(largest):
    """-> largest: None or an integer >= 1, the number of components to keep (ValueError otherwise)"""
    if largest is None:
        return None
    k = A.integer("largest", largest)
    if k < 1:
        raise ValueError(f"largest must be at least 1, got {largest!r}")
    return k


def keep_arg(keep, components, device=None):
    """-> keep: None or a contiguous CUDA uint8 tensor [components] (ValueError otherwise)"""
    if keep is None:
        return None
    return A.cuda_tensor("keep", keep, torch.uint8, (components,), f"keep: a contiguous CUDA uint8 tensor [{components}], one byte per component", device)


def largest_mask(table, k):
    """the mask uint8 [C] of the k components first in the order (triangles descending, root ascending) of a table [C, 3] = root,
    vertices, triangles (a tensor, host or device, or an array); a tensor gives a tensor on its device"""
    k = largest_arg(k)
    t = table.cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    t = t.reshape(-1, 3)
    t = t.view(np.uint32) if t.dtype == np.int32 else t
    order = np.lexsort((t[:, 0].astype(np.int64), -t[:, 2].astype(np.int64)))
    mask = np.zeros(len(t), np.uint8)
    if k is not None:
        mask[order[:k]] = 1
    return torch.from_numpy(mask).to(table.device) if isinstance(table, torch.Tensor) else mask


class Components(_lib.CtxHandle):
    """The components of meshes of up to max_vertices vertices and max_triangles triangles, on the context's stream."""
    _destroy, _signatures, _timing, _stages = "rgbid_mesh_destroy", SIGNATURES, "rgbid_mesh_timing", STAGES

    def __init__(self, ctx, max_vertices, max_triangles):
        self.max_vertices, self.max_triangles = capacity_arg(max_vertices, max_triangles)
        super().__init__(ctx)
        self._triangles = None                 # the labelled mesh: emit reads it again
        self.n_vertices = self.components = 0
        self.kept = None
        self._created(self.L.rgbid_mesh_create(C.byref(self._h), ctx._h, C.c_ulonglong(self.max_vertices), C.c_ulonglong(self.max_triangles)))

    def label(self, triangles, n_vertices, tables=True):
        """the components of the mesh `triangles` (CUDA [n_t, 3], 4-byte integers) over n_vertices vertices -> dict(components, table int32
        [C, 3] = root, vertices, triangles per component, labels int32 [n_vertices] = the component of every vertex; both hold uint32
        bits); without `tables` only the count.  The tensor is kept until the next label: select and emit read it.  Synchronises."""
        triangles, n_v = mesh_arg(triangles, n_vertices, self.max_vertices, self.max_triangles, self.ctx.device)
        self._triangles, self.kept = None, None
        n_c = C.c_ulonglong()
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_mesh_label(self._h, C.c_ulonglong(n_v), C.c_ulonglong(triangles.shape[0]), self.ptr(triangles), C.byref(n_c)))
        self._triangles, self.n_vertices, self.components = triangles, n_v, int(n_c.value)
        out = dict(components=self.components)
        if tables:
            table = torch.empty((self.components, 3), dtype=torch.int32, device=self._dev)
            labels = torch.empty((n_v,), dtype=torch.int32, device=self._dev)
            self.ctx.wait_torch_stream()   # the outputs are torch's allocations
            check(self.L.rgbid_mesh_components(self._h, self.ptr(table), self.ptr(labels)))
            self.ctx.sync()
            out.update(table=table, labels=labels)
        return out

    def select(self, min_triangles=1, keep=None):
        """keep the components of at least min_triangles triangles whose byte in `keep` (None, or CUDA uint8 [components]) is not 0 ->
        dict(components, vertices, triangles): what stays.  Synchronises."""
        n = min_triangles_arg(min_triangles)
        if self._triangles is None:
            raise ValueError("select: nothing is labelled")
        keep = keep_arg(keep, self.components, self.ctx.device)
        kc, kv, kt = C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        self.kept = None
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_mesh_select(self._h, n, self.opt_ptr(keep), C.byref(kc), C.byref(kv), C.byref(kt)))
        self.kept = dict(components=int(kc.value), vertices=int(kv.value), triangles=int(kt.value))
        return dict(self.kept)

    def emit_into(self, vertices, colours, normals, vertices_out, colours_out, normals_out, old_index_out, triangles_out):
        """the raw call: the last selection written asynchronously on the context's stream into the given CUDA tensors (or None)"""
        ptr = self.opt_ptr
        check(self.L.rgbid_mesh_emit(self._h, ptr(vertices), ptr(colours), ptr(normals), ptr(vertices_out), ptr(colours_out), ptr(normals_out),
                                     ptr(old_index_out), ptr(triangles_out), C.c_ulonglong(vertices_out.shape[0]), C.c_ulonglong(triangles_out.shape[0])))

    def emit(self, vertices, colours=None, normals=None, old_index=False):
        """the last selection of the mesh whose vertices have the positions `vertices` (CUDA float32 [n_vertices, 3]), optionally colours
        (uint8 [n_vertices, 3]) and normals (float32 [n_vertices, 3]) -> dict(vertices, colours, normals, triangles, old_index) as new CUDA
        tensors (None where there was no input; old_index int32 [kept], the kept vertices' former indices, only when asked for).
        Synchronises."""
        if self._triangles is None or self.kept is None:
            raise ValueError("emit: nothing is selected")
        dev, n = self.ctx.device, self.n_vertices
        A.rows3("vertices", vertices, torch.float32, n, dev)
        if colours is not None:
            A.rows3("colours", colours, torch.uint8, n, dev)
        if normals is not None:
            A.rows3("normals", normals, torch.float32, n, dev)
        kv, kt = self.kept["vertices"], self.kept["triangles"]
        new = lambda like, rows: None if like is None else torch.empty((rows, 3), dtype=like.dtype, device=self._dev)
        out = dict(vertices=new(vertices, kv), colours=new(colours, kv), normals=new(normals, kv),
                   triangles=torch.empty((kt, 3), dtype=torch.int32, device=self._dev),
                   old_index=torch.empty((kv,), dtype=torch.int32, device=self._dev) if old_index else None)
        self.ctx.wait_torch_stream()   # the outputs are torch's allocations
        self.emit_into(vertices, colours, normals, out["vertices"], out["colours"], out["normals"], out["old_index"], out["triangles"])
        self.ctx.sync()
        return out


def filter_components(ctx, vertices, colours, triangles, normals=None, min_triangles=1, largest=None):
    """one-shot: the mesh (vertices float32 [n, 3], colours uint8 [n, 3] or None, triangles [n_t, 3], normals float32 [n, 3] or None, CUDA
    tensors) without the components of fewer than min_triangles triangles and, with `largest` = k, without those that are not among the k
    first of all components in the order (triangles descending, root ascending) ->(vertices, colours, triangles, normals, info) with info =
    dict(components, vertices, triangles, kept_components, kept_vertices, kept_triangles)."""
    n = min_triangles_arg(min_triangles)
    k = largest_arg(largest)
    A.rows3("vertices", vertices, torch.float32)
    triangles, n_v = mesh_arg(triangles, vertices.shape[0])
    cc = Components(ctx, max(n_v, 1), max(triangles.shape[0], 1))
    try:
        lab = cc.label(triangles, n_v, tables=k is not None)
        keep = largest_mask(lab["table"], k) if k is not None else None
        kept = cc.select(n, keep)
        out = cc.emit(vertices, colours, normals)
        info = dict(components=lab["components"], vertices=n_v, triangles=int(triangles.shape[0]), kept_components=kept["components"],
                    kept_vertices=kept["vertices"], kept_triangles=kept["triangles"])
        return out["vertices"], out["colours"], out["triangles"], out["normals"], info
    finally:
        cc.close()
