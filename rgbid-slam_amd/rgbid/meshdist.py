"""Distances from points and meshes to a triangle mesh on the device (binding of include/rgbid_meshdist.h).

`Distance.plan` lays the voxel filter's grid over the triangles of a mesh and enters every triangle into the cells its box meets;
`Distance.query` finds for every query point the nearest triangle within `d_max`, the closest point on it and the distance, byte-identical
to a brute force over all triangles.  `summary` turns the distances into the figures a surface evaluation reports,
`mesh_deviation` measures two meshes against each other and `cloud_deviation` a keyframe cloud against a mesh."""
import ctypes as C

import numpy as np
import torch

from . import _args as A
from . import _lib
from . import mesh as MS
from ._lib import check, ci, f32, u64, vp

MAX_VERTICES = 1 << 31
MAX_TRIANGLES = 1 << 31
MAX_PAIRS = 1 << 31
MAX_QUERIES = 1 << 31
NONE = 0xFFFFFFFF                        # RGBID_MESHDIST_NONE
NO_REGION = 255                          # RGBID_MESHDIST_NO_REGION
MAX_CELL = 1 << 18                       # RGBID_MESHDIST_MAX_CELL
CELL_FACTOR = np.float32(1.0625)         # RGBID_MESHDIST_CELL_FACTOR: smallest cell size / d_max
MIN_DISTANCE, MAX_DISTANCE = 2.0 ** -60, 2.0 ** 60
SIGNATURES = {
    "rgbid_meshdist_create": (vp, vp, u64, u64, u64, u64),
    "rgbid_meshdist_destroy": (vp,),
    "rgbid_meshdist_plan": (vp, u64, vp, u64, vp, f32, f32, vp, vp),
    "rgbid_meshdist_query": (vp, u64, vp, vp, vp, vp, vp, vp),
    "rgbid_meshdist_query_records": (vp, u64, vp, vp, vp, vp, vp, vp),
    "rgbid_meshdist_set_query_sort": (vp, ci),
    "rgbid_meshdist_timing": (vp, ci, vp),
}
MESHDIST_EXPORTS = EXPORTS = list(SIGNATURES)
STAGES = ("box", "pairs", "sort", "cells", "query")
STATS = ("participating", "pairs", "cells", "longest_run")
OUTPUTS = ("triangle", "distance", "closest", "region", "candidates")
REGIONS = ("A", "B", "C", "AB", "AC", "BC", "face")


def capacity_arg(max_vertices, max_triangles, max_pairs, max_queries):
    """-> the four capacities of a handle: each an integer in 1 .. 2^31 (ValueError otherwise)"""
    v, t = MS.capacity_arg(max_vertices, max_triangles)
    p, q = A.integer("max_pairs", max_pairs), A.integer("max_queries", max_queries)
    return v, t, A.in_range("max_pairs", p, 1, MAX_PAIRS, "[1, 2^31]", max_pairs), A.in_range("max_queries", q, 1, MAX_QUERIES, "[1, 2^31]", max_queries)


def distance_arg(d_max):
    """-> d_max as the float32 value the library receives: finite, > 0 and in [2^-60, 2^60] (ValueError otherwise)"""
    d = A.positive32("d_max", d_max, f"d_max: a number of metres, got {d_max!r}", (bool, str, bytes))
    return A.in_range("d_max", d, MIN_DISTANCE, MAX_DISTANCE, "[2^-60, 2^60]", d_max)


def cell_arg(cell, d_max):
    """-> the cell edge as the float32 value the library forms the grid with: None gives d_max * 1.0625f; otherwise finite and at least
    that (ValueError otherwise)"""
    least = float(np.float32(distance_arg(d_max)) * CELL_FACTOR)
    if cell is None:
        return least
    c = A.positive32("cell", cell, f"cell: a number of metres, got {cell!r}", (bool, str, bytes))
    if c < least:
        raise ValueError(f"cell must be at least 1.0625 d_max = {least!r}, got {cell!r}")
    if c > MAX_DISTANCE * float(CELL_FACTOR):
        raise ValueError(f"cell must be at most 1.0625 * 2^60, got {cell!r}")
    return c


def mesh_arg(vertices, triangles, max_vertices=MAX_VERTICES, max_triangles=MAX_TRIANGLES, device=None):
    """-> (vertices, triangles): contiguous CUDA tensors float32 [n_v, 3] and 4-byte integers [n_t, 3] within the capacities, no triangles
    without vertices (ValueError otherwise)"""
    A.rows3("vertices", vertices, torch.float32, device=device)
    triangles, _ = MS.mesh_arg(triangles, vertices.shape[0], max_vertices, max_triangles, device)
    return vertices, triangles


def points_arg(points, max_queries=MAX_QUERIES, device=None):
    """-> points: a contiguous CUDA float32 tensor [n, 3] of at most max_queries rows (ValueError otherwise)"""
    A.rows3("points", points, torch.float32, device=device)
    if points.shape[0] > max_queries:
        raise ValueError(f"{points.shape[0]} points are more than {max_queries}")
    return points


def records_arg(records, max_queries=MAX_QUERIES, device=None):
    """-> records: a contiguous CUDA uint8 tensor [n, 32] of rgbid_cloud_point records, at most max_queries rows (ValueError otherwise)"""
    A.cuda_tensor("records", records, torch.uint8, (None, 32), "records: a contiguous CUDA uint8 tensor [n, 32] of rgbid_cloud_point records", device)
    if records.shape[0] > max_queries:
        raise ValueError(f"{records.shape[0]} records are more than {max_queries}")
    return records


def outputs_arg(outputs):
    """-> the requested outputs in the order of OUTPUTS: a non-empty selection of triangle, distance, closest, region, candidates
    (ValueError otherwise)"""
    if isinstance(outputs, str):
        outputs = (outputs,)
    try:
        names = list(outputs)
    except TypeError:
        raise ValueError(f"outputs: names among {OUTPUTS}, got {outputs!r}") from None
    if not names or any(not isinstance(n, str) or n not in OUTPUTS for n in names) or len(set(names)) != len(names):
        raise ValueError(f"outputs: a non-empty selection of {OUTPUTS} without repeats, got {outputs!r}")
    return tuple(n for n in OUTPUTS if n in names)


class Distance(_lib.CtxHandle):
    """The truncated nearest-triangle search over meshes of up to max_vertices vertices and max_triangles triangles whose grid holds up to
    max_pairs (cell, triangle) pairs, for up to max_queries points per call, on the context's stream."""
    _destroy, _signatures, _timing, _stages = "rgbid_meshdist_destroy", SIGNATURES, "rgbid_meshdist_timing", STAGES

    def __init__(self, ctx, max_vertices, max_triangles, max_pairs, max_queries):
        self.max_vertices, self.max_triangles, self.max_pairs, self.max_queries = capacity_arg(max_vertices, max_triangles, max_pairs, max_queries)
        super().__init__(ctx)
        self.planned = None                    # the last plan's figures
        self.needed_pairs = None               # what the last plan said it needs, also when it was refused
        self._created(self.L.rgbid_meshdist_create(C.byref(self._h), ctx._h, *(C.c_ulonglong(x) for x in (self.max_vertices, self.max_triangles,
                                                                                                            self.max_pairs, self.max_queries))))

    def sort_queries(self, enable=True):
        """walk the queries of the following calls in the order of their cells (the default) or in input order; the outputs are the same"""
        check(self.L.rgbid_meshdist_set_query_sort(self._h, int(bool(enable))))

    def plan(self, vertices, triangles, d_max, cell=None):
        """the grid of the mesh (CUDA float32 [n_v, 3], 4-byte integers [n_t, 3]) for queries up to d_max metres, with cells of `cell`
        metres (None: 1.0625 d_max) -> dict(grid = min_b[3] + div_b[3], participating, pairs, cells, longest_run, d_max, cell).  The
        corners are copied: the tensors are free afterwards.  A mesh that needs more than max_pairs pairs raises, with the needed count
        in `.needed_pairs`.  Synchronises."""
        d = distance_arg(d_max)
        c = cell_arg(cell, d)
        vertices, triangles = mesh_arg(vertices, triangles, self.max_vertices, self.max_triangles, self.ctx.device)
        self.planned, self.needed_pairs = None, None
        grid, stats = (C.c_longlong * 6)(), (C.c_ulonglong * 4)()
        self.ctx.wait_torch_stream()
        err = self.L.rgbid_meshdist_plan(self._h, C.c_ulonglong(vertices.shape[0]), self.ptr(vertices), C.c_ulonglong(triangles.shape[0]),
                                         self.ptr(triangles), C.c_float(d), C.c_float(0.0 if cell is None else c), grid, stats)
        self.needed_pairs = int(stats[1])
        if err and self.needed_pairs > self.max_pairs:
            raise _lib.RgbidError(f"the mesh needs {self.needed_pairs} (cell, triangle) pairs, the handle holds {self.max_pairs}")
        check(err)
        self.planned = dict(grid=[int(x) for x in grid], **dict(zip(STATS, (int(x) for x in stats))), d_max=d, cell=c)
        return dict(self.planned)

    def query_into(self, points, triangle=None, distance=None, closest=None, region=None, candidates=None, records=False):
        """the raw call: the queries (float32 [n, 3], or with `records` uint8 [n, 32]) against the last plan, written asynchronously on
        the context's stream into the given CUDA tensors (or None)"""
        ptr = self.opt_ptr
        f = self.L.rgbid_meshdist_query_records if records else self.L.rgbid_meshdist_query
        check(f(self._h, C.c_ulonglong(points.shape[0]), ptr(points), ptr(triangle), ptr(distance), ptr(closest), ptr(region), ptr(candidates)))

    def _query(self, points, outputs, records):
        outputs = outputs_arg(outputs)
        if self.planned is None:
            raise ValueError("query: nothing is planned")
        n = points.shape[0]
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=self._dev)
        shapes = dict(triangle=((n,), torch.int32), distance=((n,), torch.float32), closest=((n, 3), torch.float32), region=((n,), torch.uint8),
                      candidates=((n,), torch.int32))
        out = {k: new(*shapes[k]) for k in outputs}
        self.ctx.wait_torch_stream()   # the outputs are torch's allocations
        self.query_into(points, records=records, **out)
        self.ctx.sync()
        return out

    def query(self, points, outputs=("triangle", "distance")):
        """the nearest triangle within d_max of every point (CUDA float32 [n, 3]) -> dict of new CUDA tensors: triangle int32 [n] (uint32
        bits, -1 = none), distance float32 [n] (NaN = none), closest float32 [n, 3], region uint8 [n] (0 .. 6 = A B C AB AC BC face, 255
        = none), candidates int32 [n]; only those asked for.  Synchronises."""
        return self._query(points_arg(points, self.max_queries, self.ctx.device), outputs, False)

    def query_records(self, records, outputs=("triangle", "distance")):
        """the same for the positions of rgbid_cloud_point records (CUDA uint8 [n, 32])"""
        return self._query(records_arg(records, self.max_queries, self.ctx.device), outputs, True)


def summary(distance):
    """the figures of a distance tensor (float32 [n], NaN = no triangle within d_max) -> dict(queries, matched, mean, rms, median, p90,
    max) over the matched queries, computed on the tensor's device; median and p90 are nearest-rank quantiles; NaN where nothing matched.
    A report, not part of the byte contract."""
    if not (isinstance(distance, torch.Tensor) and distance.dtype == torch.float32 and distance.dim() == 1):
        raise ValueError("distance: a float32 tensor [n]")
    d = distance[~torch.isnan(distance)].to(torch.float64)
    n, m = int(distance.shape[0]), int(d.shape[0])
    if m == 0:
        nan = float("nan")
        return dict(queries=n, matched=0, mean=nan, rms=nan, median=nan, p90=nan, max=nan)
    s = torch.sort(d).values
    rank = lambda q10: float(s[(q10 * m + 9) // 10 - 1])
    return dict(queries=n, matched=m, mean=float(d.mean()), rms=float(torch.sqrt((d * d).mean())), median=rank(5), p90=rank(9), max=float(s[-1]))


def pair_bound(triangles, factor=8):
    """a first guess of max_pairs for a mesh of this many triangles; `deviation` grows it when the plan asks for more"""
    return max(int(triangles) * factor, 1024)


def _planned(ctx, vertices, triangles, d_max, cell, max_queries):
    """a Distance with the mesh planned, its pair capacity grown once to what the plan asks for"""
    vertices, triangles = mesh_arg(vertices, triangles)
    n_v, n_t = max(vertices.shape[0], 1), max(triangles.shape[0], 1)
    dist = Distance(ctx, n_v, n_t, min(pair_bound(n_t), MAX_PAIRS), max(int(max_queries), 1))
    try:
        try:
            dist.plan(vertices, triangles, d_max, cell)
        except _lib.RgbidError:
            need = dist.needed_pairs
            if need is None or not dist.max_pairs < need <= MAX_PAIRS:
                raise
            dist.close()
            dist = Distance(ctx, n_v, n_t, need, max(int(max_queries), 1))
            dist.plan(vertices, triangles, d_max, cell)
    except Exception:
        dist.close()
        raise
    return dist


def point_deviation(ctx, points, vertices, triangles, d_max, cell=None):
    """one-shot: summary of the distances of the points (CUDA float32 [n, 3]) to the mesh, truncated at d_max"""
    points_arg(points)
    dist = _planned(ctx, vertices, triangles, d_max, cell, points.shape[0])
    try:
        return summary(dist.query(points, ("distance",))["distance"])
    finally:
        dist.close()


def mesh_deviation(ctx, va, ta, vb, tb, d_max, cell=None):
    """two meshes measured against each other (vertices CUDA float32 [n, 3], triangles [n_t, 3]) -> dict(a_to_b, b_to_a, hausdorff):
    the `summary` of the distances of A's vertices to the surface of B and of B's vertices to the surface of A, each truncated at d_max (a
    vertex farther away than d_max from the other mesh is unmatched and enters no figure), and the larger of the two `max`: the
    vertex-sampled symmetric Hausdorff distance, truncated at d_max.  Vertex-sampled: only the vertices are measured, not points inside
    the triangles, so a coarse mesh is sampled coarsely."""
    va, ta = mesh_arg(va, ta)
    vb, tb = mesh_arg(vb, tb)
    distance_arg(d_max)
    a_to_b = point_deviation(ctx, va, vb, tb, d_max, cell)
    b_to_a = point_deviation(ctx, vb, va, ta, d_max, cell)
    both = [x["max"] for x in (a_to_b, b_to_a) if x["matched"]]
    return dict(a_to_b=a_to_b, b_to_a=b_to_a, hausdorff=max(both) if both else float("nan"))


def cloud_deviation(ctx, records, vertices, triangles, d_max, cell=None):
    """a cloud of rgbid_cloud_point records (CUDA uint8 [n, 32]) measured against a mesh -> the `summary` of the distances of the records'
    positions to the surface, truncated at d_max"""
    records_arg(records)
    dist = _planned(ctx, vertices, triangles, d_max, cell, records.shape[0])
    try:
        return summary(dist.query_records(records, ("distance",))["distance"])
    finally:
        dist.close()


def summary_line(s):
    """a `summary` as the command-line tools print it"""
    return (f"{s['matched']} of {s['queries']} matched, mean {s['mean']:.6f} m, rms {s['rms']:.6f} m, median {s['median']:.6f} m, "
            f"90 % {s['p90']:.6f} m, max {s['max']:.6f} m")
