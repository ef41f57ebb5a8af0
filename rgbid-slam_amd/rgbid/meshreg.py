"""Point sets and meshes registered to a triangle mesh on the device (binding of include/rgbid_meshreg.h).

`Registration.target` plans the truncated nearest-triangle search of `rgbid.meshdist` over the target mesh and computes its triangles'
normals; `Registration.align` runs point-to-plane ICP from any number of starting poses at once, every iteration enqueued without a host
wait, byte-identical to tests/meshreg_mirror.py.  `choose` picks a start from the records, `principal_starts`
proposes four starts from the principal axes, and `register_points` / `register_mesh` do the whole evaluation: register, then measure with
`meshdist.mesh_deviation` before and after."""
import ctypes as C
import math

import numpy as np
import torch

from . import _args as A
from . import _lib
from . import meshdist as MD
from ._lib import check, ci, cu, f32, f64, u64, vp

MAX_STARTS = 256
MAX_QUERIES = 1 << 31                    # RGBID_MESHREG_MAX_QUERIES: the bound of max_points * max_starts
MAX_LEVELS, MAX_ITERATIONS, TERMS = 4, 256, 28
RUNNING, CONVERGED, FEW, SINGULAR = 0, 1, 2, 3
STATUS = ("running", "converged", "few", "singular")                                                                                   # RGBID_MESHREG_*
SIGNATURES = {
    "rgbid_meshreg_create": (vp, vp, u64, u64, u64, u64, u64),
    "rgbid_meshreg_destroy": (vp,),
    "rgbid_meshreg_target": (vp, u64, vp, u64, vp, f32, f32, vp, vp),
    "rgbid_meshreg_align": (vp, u64, vp, ci, vp, f32, f64, f64, cu, ci, vp, vp),
    "rgbid_meshreg_align_records": (vp, u64, vp, ci, vp, f32, f64, f64, cu, ci, vp, vp),
    "rgbid_meshreg_apply": (vp, u64, vp, vp, vp, vp, vp),
    "rgbid_meshreg_set_query_sort": (vp, ci),
    "rgbid_meshreg_timing": (vp, ci, vp),
}
MESHREG_EXPORTS = EXPORTS = list(SIGNATURES)
STAGES = ("transform", "query", "system", "solve")
# rgbid_meshreg_result: 560 bytes
RESULT = np.dtype([("pose", "<f8", (12,)), ("status", "<i4"), ("iterations", "<i4"), ("used", "<u4", (2,)), ("sums", "<f8", (2, TERMS))])


class Level(C.Structure):
    """rgbid_meshreg_level"""
    _fields_ = [("stride", C.c_int), ("iterations", C.c_int), ("reach", C.c_float)]


def capacity_arg(max_vertices, max_triangles, max_pairs, max_points, max_starts):
    """-> the five capacities of a handle: the target's as meshdist.capacity_arg takes them, max_points >= 1, max_starts in 1 .. 256 and
    max_points * max_starts <= 2^31 (ValueError otherwise)"""
    n = A.integer_in("max_points", max_points, 1, MAX_QUERIES, "[1, 2^31]")
    s = A.integer_in("max_starts", max_starts, 1, MAX_STARTS, f"[1, {MAX_STARTS}]")
    if n * s > MAX_QUERIES:
        raise ValueError(f"max_points * max_starts must be at most 2^31, got {max_points!r} * {max_starts!r}")
    v, t, p, _ = MD.capacity_arg(max_vertices, max_triangles, max_pairs, n * s)
    return v, t, p, n, s


def starts_arg(R, t, max_starts=MAX_STARTS):
    """the starting poses R [V, 3, 3] (or [3, 3]) and t [V, 3] (or [3]), source -> target -> float64 [V, 12] = R00 .. R22 tx ty tz:
    1 <= V <= max_starts, every entry finite (ValueError otherwise)"""
    try:
        R = np.asarray(R, np.float64).reshape(-1, 9)
        t = np.asarray(t, np.float64).reshape(-1, 3)
    except (TypeError, ValueError):
        raise ValueError("R: [V, 3, 3] and t: [V, 3] numbers") from None
    if len(R) < 1 or len(R) != len(t):
        raise ValueError(f"R and t must hold the same number (>= 1) of starts, got {len(R)} and {len(t)}")
    if len(R) > max_starts:
        raise ValueError(f"{len(R)} starts are more than {max_starts}")
    if not (np.isfinite(R).all() and np.isfinite(t).all()):
        raise ValueError("poses must be finite")
    return np.ascontiguousarray(np.concatenate([R, t], 1))


def default_levels(d_max):
    """three levels over every fourth, every second and every point, the reach halved from d_max each time"""
    d = MD.distance_arg(d_max)
    return ((4, 15, d), (2, 15, d / 2), (1, 20, d / 4))


def levels_arg(levels, d_max):
    """-> the levels as a tuple of (stride, iterations, reach): 1 .. 4 triples, stride >= 1, iterations >= 1 and at most 256 in all, the
    reach a float32 value with 0 < reach <= d_max; None gives default_levels(d_max) (ValueError otherwise)"""
    d = MD.distance_arg(d_max)
    if levels is None:
        levels = default_levels(d)
    try:
        lv = [tuple(l) for l in levels]
    except TypeError:
        raise ValueError(f"levels: triples (stride, iterations, reach), got {levels!r}") from None
    if not 1 <= len(lv) <= MAX_LEVELS or any(len(l) != 3 for l in lv):
        raise ValueError(f"levels: 1 .. {MAX_LEVELS} triples (stride, iterations, reach), got {levels!r}")
    lv = tuple((A.integer("stride", s), A.integer("iterations", n), A.positive32("reach", r, f"reach: a number of metres, got {r!r}", (bool, str, bytes)))
               for s, n, r in lv)
    if any(not 1 <= s < 1 << 31 for s, _, _ in lv):
        raise ValueError(f"a stride must be at least 1, got {levels!r}")
    if any(n < 1 for _, n, _ in lv) or sum(n for _, n, _ in lv) > MAX_ITERATIONS:
        raise ValueError(f"every level needs at least 1 iteration and all together at most {MAX_ITERATIONS}, got {levels!r}")
    if any(r > d for _, _, r in lv):
        raise ValueError(f"a reach must be at most d_max = {d!r}, got {levels!r}")
    return lv


def params_arg(huber, damping, eps, min_points):
    """-> (huber, damping, eps, min_points) as the library takes them: huber a finite float32 > 0, damping finite and >= 0, eps finite and
    > 0, min_points an integer in 6 .. 2^32 - 1 (ValueError otherwise)"""
    h, d, e, n = A.finite32("huber", huber), A.finite64("damping", damping), A.finite64("eps", eps), A.integer("min_points", min_points)
    if not h > 0:
        raise ValueError(f"huber must be > 0, got {huber!r}")
    if not d >= 0:
        raise ValueError(f"damping must be >= 0, got {damping!r}")
    if not e > 0:
        raise ValueError(f"eps must be > 0, got {eps!r}")
    if not 6 <= n < 1 << 32:
        raise ValueError(f"min_points must be at least 6, got {min_points!r}")
    return h, d, e, n


def result_dict(res):
    """the records of rgbid_meshreg_align (RESULT [V]) -> dict(R [V, 3, 3], t [V, 3], status, iterations [V], used [V, 2],
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


def rms(result):
    """the residual rms (m) of the last system of every start of an `align` result, NaN where no point was used"""
    used, err = np.asarray(result["used"])[:, 1].astype(np.float64), np.asarray(result["error"])[:, 1]
    with np.errstate(all="ignore"):
        return np.sqrt(err / used)


def choose(result):
    """the start to take from an `align` result: among those that ended converged or running with a used point, the one with the largest
    last `used`, then the smallest last rms, then the smallest index; None when there is none"""
    r = rms(result)
    ok = [v for v in range(len(r)) if int(result["status"][v]) in (RUNNING, CONVERGED) and int(result["used"][v][1]) > 0]
    return min(ok, key=lambda v: (-int(result["used"][v][1]), float(r[v]), v)) if ok else None


def principal_starts(points, vertices):
    """four starts for `align`: the proper rotations that map the principal axes of the points (CUDA float32 [n, 3], the source) onto those
    of the vertices (the target), the centroids matched -> (R float64 [4, 3, 3], t float64 [4, 3]).  The axes' signs are undetermined, so
    the four sign choices with determinant +1 are all proposed and `choose` takes the winner.  float64 torch on the tensors' device, over
    the finite rows; a report, not part of the byte contract."""
    A.rows3("points", points, torch.float32)
    A.rows3("vertices", vertices, torch.float32)

    def frame(x):
        x = x[torch.isfinite(x).all(1)].to(torch.float64)
        if x.shape[0] < 3:
            raise ValueError("principal_starts needs at least 3 finite rows on either side")
        c = x.mean(0)
        _, E = torch.linalg.eigh((x - c).T @ (x - c) / x.shape[0])      # ascending eigenvalues, columns
        if torch.linalg.det(E) < 0:
            E = E * torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64, device=E.device)
        return c.cpu().numpy(), E.cpu().numpy()

    cs, Es = frame(points)
    ct, Et = frame(vertices)
    R = np.stack([Et @ np.diag(s) @ Es.T for s in ((1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))])
    return R, np.stack([ct - r @ cs for r in R])


class Registration(_lib.CtxHandle):
    """Point-to-plane ICP of up to max_points points from up to max_starts starts against meshes of up to max_vertices vertices and
    max_triangles triangles whose grid holds up to max_pairs (cell, triangle) pairs, on the context's stream."""
    _destroy, _signatures, _timing, _stages = "rgbid_meshreg_destroy", SIGNATURES, "rgbid_meshreg_timing", STAGES

    def __init__(self, ctx, max_vertices, max_triangles, max_pairs, max_points, max_starts):
        self.max_vertices, self.max_triangles, self.max_pairs, self.max_points, self.max_starts = capacity_arg(max_vertices, max_triangles, max_pairs,
                                                                                                                 max_points, max_starts)
        super().__init__(ctx)
        self.planned = None                    # the last target's figures
        self.needed_pairs = None               # what the last target said it needs, also when it was refused
        self._created(self.L.rgbid_meshreg_create(C.byref(self._h), ctx._h, *(C.c_ulonglong(x) for x in (self.max_vertices, self.max_triangles,
                                                                                                           self.max_pairs, self.max_points, self.max_starts))))

    def sort_queries(self, enable=True):
        """walk the search's queries of the following calls in the order of their cells (the default) or in input order; the results are
        the same"""
        check(self.L.rgbid_meshreg_set_query_sort(self._h, int(bool(enable))))

    def target(self, vertices, triangles, d_max, cell=None):
        """the mesh to register to (CUDA float32 [n_v, 3], 4-byte integers [n_t, 3]), searched up to d_max metres with cells of `cell`
        metres (None: 1.0625 d_max) -> the figures of meshdist.Distance.plan.  The mesh is copied: the tensors are free afterwards.  A mesh
        that needs more than max_pairs pairs raises, with the needed count in `.needed_pairs`.  Synchronises."""
        d = MD.distance_arg(d_max)
        c = MD.cell_arg(cell, d)
        vertices, triangles = MD.mesh_arg(vertices, triangles, self.max_vertices, self.max_triangles, self.ctx.device)
        self.planned, self.needed_pairs = None, None
        grid, stats = (C.c_longlong * 6)(), (C.c_ulonglong * 4)()
        self.ctx.wait_torch_stream()
        err = self.L.rgbid_meshreg_target(self._h, C.c_ulonglong(vertices.shape[0]), self.ptr(vertices), C.c_ulonglong(triangles.shape[0]),
                                          self.ptr(triangles), C.c_float(d), C.c_float(0.0 if cell is None else c), grid, stats)
        self.needed_pairs = int(stats[1])
        if err and self.needed_pairs > self.max_pairs:
            raise _lib.RgbidError(f"the mesh needs {self.needed_pairs} (cell, triangle) pairs, the handle holds {self.max_pairs}")
        check(err)
        self.planned = dict(grid=[int(x) for x in grid], **dict(zip(MD.STATS, (int(x) for x in stats))), d_max=d, cell=c)
        return dict(self.planned)

    def _align_args(self, R, t, levels, huber, damping, eps, min_points):
        """the alignment's arguments as the library takes them (ValueError for what it would refuse)"""
        if self.planned is None:
            raise ValueError("align: there is no target")
        d = self.planned["d_max"]
        return (starts_arg(R, t, self.max_starts), levels_arg(levels, d)) + params_arg(d if huber is None else huber, damping, eps, min_points)

    def align_into(self, points, R, t, levels, huber, damping, eps, min_points, result, records=False):
        """the raw call: checked arguments, the records written asynchronously on the context's stream into `result`, a contiguous CUDA
        uint8 tensor of 560 bytes per start; points float32 [n, 3], or with `records` uint8 [n, 32]"""
        poses, lv, h, d, e, n = self._align_args(R, t, levels, huber, damping, eps, min_points)
        points = (MD.records_arg if records else MD.points_arg)(points, self.max_points, self.ctx.device)
        V = len(poses)
        if not (isinstance(result, torch.Tensor) and result.is_cuda and result.dtype == torch.uint8 and result.is_contiguous()
                and result.numel() == V * RESULT.itemsize and result.device.index == self.ctx.device and result.data_ptr() % 8 == 0):
            raise ValueError(f"result: a contiguous CUDA uint8 tensor of {V} x {RESULT.itemsize} bytes on device {self.ctx.device}")
        lv_arr = (Level * len(lv))(*[Level(s, k, r) for s, k, r in lv])
        f = self.L.rgbid_meshreg_align_records if records else self.L.rgbid_meshreg_align
        check(f(self._h, C.c_ulonglong(points.shape[0]), self.ptr(points), V, poses.ctypes.data_as(C.c_void_p), C.c_float(h), C.c_double(d),
                C.c_double(e), n, len(lv), lv_arr, C.c_void_p(result.data_ptr())))

    def _align(self, points, R, t, levels, huber, damping, eps, min_points, records):
        V = len(self._align_args(R, t, levels, huber, damping, eps, min_points)[0])
        (MD.records_arg if records else MD.points_arg)(points, self.max_points, self.ctx.device)
        result = torch.empty((V * RESULT.itemsize,), dtype=torch.uint8, device=self._dev)
        self.ctx.wait_torch_stream()   # the points and the result are torch's
        self.align_into(points, R, t, levels, huber, damping, eps, min_points, result, records)
        self.ctx.sync()
        return result_dict(result.cpu().numpy().view(RESULT))

    def align(self, points, R, t, levels=None, huber=None, damping=0.0, eps=1e-7, min_points=6):
        """register the points (CUDA float32 [n, 3]) to the target from the starts R [V, 3, 3], t [V, 3] (source -> target), over the
        `levels` (stride, iterations, reach) in order (None: every fourth, second and every point with the reach d_max, d_max / 2,
        d_max / 4), with the Huber threshold `huber` in metres (None: d_max), the damping H_jj (1 + damping), the step bound `eps` that
        ends a level, and at least `min_points` used points -> dict(R [V, 3, 3], t [V, 3] float64, status [V] (an index into STATUS),
        iterations [V], used [V, 2], H [V, 2, 6, 6], b [V, 2, 6], error [V, 2]: the normal equations H delta = -b for delta = (v, omega)
        in the target's frame and the weighted squared residual, of the first and of the last system built).  Synchronises."""
        return self._align(points, R, t, levels, huber, damping, eps, min_points, False)

    def align_records(self, records, R, t, levels=None, huber=None, damping=0.0, eps=1e-7, min_points=6):
        """the same for the positions of rgbid_cloud_point records (CUDA uint8 [n, 32])"""
        return self._align(records, R, t, levels, huber, damping, eps, min_points, True)

    def apply(self, points, R, t, normals=None):
        """the points (CUDA float32 [n, 3]) moved by the pose R [3, 3], t [3] -> a new tensor; with normals (float32 [n, 3]) the pair
        (points, rotated normals, not renormalised).  Synchronises."""
        pose = starts_arg(R, t, 1)[0]
        A.rows3("points", points, torch.float32, device=self.ctx.device)
        if normals is not None:
            A.rows3("normals", normals, torch.float32, points.shape[0], self.ctx.device)
        out = torch.empty_like(points)
        nout = None if normals is None else torch.empty_like(normals)
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_meshreg_apply(self._h, C.c_ulonglong(points.shape[0]), self.ptr(points), self.opt_ptr(normals),
                                         pose.ctypes.data_as(C.c_void_p), self.ptr(out), self.opt_ptr(nout)))
        self.ctx.sync()
        return out if normals is None else (out, nout)


def _targeted(ctx, vertices, triangles, d_max, cell, max_points, max_starts):
    """a Registration with the target set, its pair capacity grown once to what the plan asks for"""
    vertices, triangles = MD.mesh_arg(vertices, triangles)
    n_v, n_t = max(vertices.shape[0], 1), max(triangles.shape[0], 1)
    reg = Registration(ctx, n_v, n_t, min(MD.pair_bound(n_t), MD.MAX_PAIRS), max(int(max_points), 1), max_starts)
    try:
        try:
            reg.target(vertices, triangles, d_max, cell)
        except _lib.RgbidError:
            need = reg.needed_pairs
            if need is None or not reg.max_pairs < need <= MD.MAX_PAIRS:
                raise
            reg.close()
            reg = Registration(ctx, n_v, n_t, need, max(int(max_points), 1), max_starts)
            reg.target(vertices, triangles, d_max, cell)
    except Exception:
        reg.close()
        raise
    return reg


def _starts(starts, points, vertices):
    if starts is None:
        return np.eye(3)[None], np.zeros((1, 3))
    if isinstance(starts, str):
        if starts == "identity":
            return np.eye(3)[None], np.zeros((1, 3))
        if starts == "principal":
            return principal_starts(points, vertices)
        raise ValueError(f"starts: None, 'identity', 'principal' or (R, t), got {starts!r}")
    try:
        R, t = starts
    except (TypeError, ValueError):
        raise ValueError(f"starts: None, 'identity', 'principal' or (R, t), got {starts!r}") from None
    return R, t


def register_points(ctx, points, vertices, triangles, d_max, starts=None, cell=None, **align):
    """one-shot: the points (CUDA float32 [n, 3]) registered to the mesh from `starts` (None or "identity", "principal", or (R, t)); the
    keywords are `Registration.align`'s -> dict(R [3, 3], t [3], start, status (a word of STATUS), iterations, used, rms: of the chosen
    start; result: every start's record as `align` returns it; points: the moved points, a new CUDA tensor), or with R = None and no points
    when no start ended converged or running"""
    MD.points_arg(points)
    R0, t0 = _starts(starts, points, vertices)
    poses = starts_arg(R0, t0)
    reg = _targeted(ctx, vertices, triangles, d_max, cell, points.shape[0], len(poses))
    try:
        res = reg.align(points, poses[:, :9], poses[:, 9:], **align)
        v = choose(res)
        if v is None:
            return dict(R=None, t=None, start=None, status=None, iterations=None, used=None, rms=None, result=res, points=None)
        return dict(R=res["R"][v], t=res["t"][v], start=v, status=STATUS[int(res["status"][v])], iterations=int(res["iterations"][v]),
                    used=int(res["used"][v][1]), rms=float(rms(res)[v]), result=res, points=reg.apply(points, res["R"][v], res["t"][v]))
    finally:
        reg.close()


def register_mesh(ctx, va, ta, vb, tb, d_max, starts=None, cell=None, **align):
    """one-shot: mesh A (vertices CUDA float32 [n, 3], triangles [n_t, 3]) registered to mesh B by its vertices -> register_points' dict
    (`points` are A's moved vertices) with before and after: meshdist.mesh_deviation of the two meshes as given and with A moved (after is
    None when no start was chosen)"""
    va, ta = MD.mesh_arg(va, ta)
    vb, tb = MD.mesh_arg(vb, tb)
    out = register_points(ctx, va, vb, tb, d_max, starts, cell, **align)
    out["before"] = MD.mesh_deviation(ctx, va, ta, vb, tb, d_max, cell)
    out["after"] = None if out["points"] is None else MD.mesh_deviation(ctx, out["points"], ta, vb, tb, d_max, cell)
    return out


def pose_lines(reg):
    """a register_points / register_mesh result as the command-line tools print it: the status line and the pose's three rows"""
    if reg["R"] is None:
        return ["registration: no start ended converged or running"]
    angle = math.acos(min(1.0, max(-1.0, (float(np.trace(reg["R"])) - 1.0) / 2.0)))
    lines = [f"registration: start {reg['start']} {reg['status']} after {reg['iterations']} systems, {reg['used']} points used, "
             f"rms {reg['rms']:.6f} m, rotation {angle:.6f} rad, translation {float(np.linalg.norm(reg['t'])):.6f} m"]
    return lines + ["  " + " ".join(f"{x: .9f}" for x in list(reg["R"][i]) + [reg["t"][i]]) for i in range(3)]
