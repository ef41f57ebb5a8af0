"""numpy restatement of the registration contract (include/rgbid_meshreg.h): the judge of csrc/kernels_meshreg.hip.
The search is tests/meshdist_mirror.py's brute force, the tree, the solve and the update are tests/align_mirror.py's; every double is formed
by float64 operations in exactly the order of the header, integers and comparisons decide.  `align` is vectorised over the points of a
level; `align_loop` is the plain scalar loop of the same contract that the CPU tests hold it against."""
import math

import numpy as np

from tests import align_mirror as AM
from tests import meshdist_mirror as DM

F = np.float32
D = np.float64
RUNNING, CONVERGED, FEW, SINGULAR = AM.RUNNING, AM.CONVERGED, AM.FEW, AM.SINGULAR
STATUS_NAMES = AM.STATUS_NAMES
TERMS = AM.TERMS
PAIRS = AM.PAIRS
NONE = DM.NONE
MAX_LEVELS, MAX_ITERATIONS, MAX_STARTS = 4, 256, 256
RESULT_DTYPE = AM.RESULT_DTYPE                                    # rgbid_meshreg_result is laid out as rgbid_tsdf_align_result
NAN64 = np.array([AM.NAN_BITS], np.uint64).view(D)[0]


class Target:
    """step 1: the mesh, d_max, the triangles' normals (float64 [n_t, 3], NaN rows without one) and which triangles have one"""

    def __init__(self, vertices, triangles, d_max):
        self.v, self.t = DM.prepare(vertices, triangles)
        self.d_max = DM.distance32(d_max)
        self.normals, self.has = normals(self.v, self.t)
        self.block = max(256, (1 << 20) // max(len(self.t), 1))   # queries per round of the brute force

    def query(self, p):
        return DM.query(self.v, self.t, p, self.d_max, block=self.block)

    def query_loop(self, p):
        return DM.query_loop(self.v, self.t, p, self.d_max)


def normals(v, t):
    """step 1 -> (float64 [n_t, 3], NaN where the triangle has no normal; bool [n_t])"""
    c, part, _, _ = DM.corners(v, t)
    c = c.astype(D)
    with np.errstate(all="ignore"):
        ab, ac = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
        m = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2], ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], 1)
        l2 = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]
        has = part & (l2 > 0) & np.isfinite(l2)
        n = m / np.sqrt(l2)[:, None]
    n[~has] = NAN64
    return n, has


def transform(pose, pts):
    """step 4: the 12 doubles on float32 [n, 3] -> float32 [n, 3]"""
    m = np.asarray(pose, D)
    x = np.asarray(pts, F).reshape(-1, 3).astype(D)
    with np.errstate(all="ignore"):
        return np.stack([(((m[3 * k] * x[:, 0] + m[3 * k + 1] * x[:, 1]) + m[3 * k + 2] * x[:, 2]) + m[9 + k]).astype(F) for k in range(3)], 1)


def apply(pose, pts, nrm=None):
    """step 12 -> the points, or (points, normals)"""
    out = transform(pose, pts)
    if nrm is None:
        return out
    m = np.asarray(pose, D)
    x = np.asarray(nrm, F).reshape(-1, 3).astype(D)
    with np.errstate(all="ignore"):
        return out, np.stack([((m[3 * k] * x[:, 0] + m[3 * k + 1] * x[:, 1]) + m[3 * k + 2] * x[:, 2]).astype(F) for k in range(3)], 1)


def point_values(tg, p, reach, huber):
    """steps 5 and 6 for the transformed points p (float32 [n, 3]) -> dict(used bool [n], f, w float64 [n], J [6] of float64 [n],
    triangle, distance, closest: the search's answers)"""
    q = tg.query(p)
    won = q["triangle"] != NONE
    ti = np.where(won, q["triangle"], 0).astype(np.int64)
    with np.errstate(invalid="ignore"):
        used = won & (q["distance"] <= F(reach))
    if len(tg.t):
        used &= tg.has[ti]
        n = tg.normals[ti]
    else:
        n = np.zeros((len(p), 3), D)
    with np.errstate(all="ignore"):
        P, r = p.astype(D), q["closest"].astype(D)
        e = P - r
        f = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
        J = [n[:, 0], n[:, 1], n[:, 2], P[:, 1] * n[:, 2] - P[:, 2] * n[:, 1], P[:, 2] * n[:, 0] - P[:, 0] * n[:, 2], P[:, 0] * n[:, 1] - P[:, 1] * n[:, 0]]
        h = D(F(huber))
        w = np.where(np.abs(f) <= h, D(1), h / np.abs(f))
    return dict(used=used, f=f, w=w, J=J, triangle=q["triangle"], distance=q["distance"], closest=q["closest"])


def terms_of(pv):
    """step 6 -> float64 [28, n], +0.0 where the point is not used"""
    with np.errstate(all="ignore"):
        a = [pv["w"] * j for j in pv["J"]]
        t = [a[i] * pv["J"][j] for i, j in PAIRS] + [a[i] * pv["f"] for i in range(6)] + [(pv["w"] * pv["f"]) * pv["f"]]
    return np.where(pv["used"][None], np.stack(t), D(0))


def group_lanes(x):
    """step 7: [..., n_l] -> [..., groups, 64]: 64 consecutive lattice indices per group, +0.0 beyond n_l; at least one group"""
    n = x.shape[-1]
    g = max((n + 63) // 64, 1)
    pad = np.zeros(x.shape[:-1] + (g * 64,), x.dtype)
    pad[..., :n] = x
    return pad.reshape(x.shape[:-1] + (g, 64))


def system(tg, pts, pose, stride, reach, huber):
    """steps 3 - 7 for one start -> (used count, the 28 sums as float64)"""
    p = transform(pose, np.asarray(pts, F).reshape(-1, 3)[::stride])
    pv = point_values(tg, p, reach, huber)
    return int(pv["used"].sum()), AM.reduce_tiles(AM.tree64(group_lanes(terms_of(pv))))


def _run(system_fn, R, t, levels, damping, eps, min_points):
    """steps 8 - 11 around system_fn(pose, stride, reach) -> the records"""
    V = len(R)
    out = np.zeros(V, RESULT_DTYPE)
    for v in range(V):
        pose = np.concatenate([R[v].reshape(9), t[v]]).astype(D)
        status, its = RUNNING, 0
        for stride, iters, reach in levels:
            if status == CONVERGED:
                status = RUNNING
            for _ in range(iters):
                if status != RUNNING:
                    break
                used, sums = system_fn(pose, stride, reach)
                if its == 0:
                    out[v]["used"][0], out[v]["sums"][0] = used, AM.one_nan(sums)
                out[v]["used"][1], out[v]["sums"][1] = used, AM.one_nan(sums)
                its += 1
                if used < min_points:
                    status = FEW
                    break
                delta = AM.solve(sums, damping)
                if delta is None:
                    status = SINGULAR
                    break
                pose = AM.update(pose, delta)
                if max(abs(x) for x in delta) < eps:
                    status = CONVERGED
        out[v]["pose"], out[v]["status"], out[v]["iterations"] = AM.one_nan(pose), status, its
    return out


def default_levels(d_max):
    d = float(F(d_max))
    return ((4, 15, d), (2, 15, d / 2), (1, 20, d / 4))


def levels_of(levels, d_max):
    """step 3's table as the library receives it (the reach as float32); ValueError as the binding raises it"""
    lv = [(int(s), int(n), float(F(r))) for s, n, r in (default_levels(d_max) if levels is None else levels)]
    if not 1 <= len(lv) <= MAX_LEVELS or any(s < 1 or n < 1 for s, n, _ in lv) or sum(n for _, n, _ in lv) > MAX_ITERATIONS:
        raise ValueError("levels out of range")
    if any(not (math.isfinite(r) and 0 < r <= float(F(d_max))) for _, _, r in lv):
        raise ValueError("a reach out of range")
    return lv


def align(tg, points, R, t, levels=None, huber=None, damping=0.0, eps=1e-7, min_points=6):
    """steps 2 - 11 for V starts against the Target tg -> the result records (RESULT_DTYPE [V]) as the device writes them"""
    R = np.asarray(R, D).reshape(-1, 3, 3); t = np.asarray(t, D).reshape(-1, 3)
    huber = tg.d_max if huber is None else huber
    pts = np.asarray(points, F).reshape(-1, 3)
    fn = lambda pose, stride, reach: system(tg, pts, pose, stride, reach, huber)
    return _run(fn, R, t, levels_of(levels, tg.d_max), damping, eps, min_points)


as_dict = AM.as_dict


def rms(res):
    """the residual rms of the last system of each record (NaN without a used point)"""
    with np.errstate(all="ignore"):
        return np.sqrt(res["sums"][:, 1, 27] / res["used"][:, 1])


def choose(res):
    """the start rgbid.meshreg.choose picks from the records, or None"""
    r = rms(res)
    ok = [v for v in range(len(res)) if res["status"][v] in (RUNNING, CONVERGED) and res["used"][v, 1] > 0]
    return min(ok, key=lambda v: (-int(res["used"][v, 1]), float(r[v]), v)) if ok else None


# ---- the scalar loop ----------------------------------------------------------------------------------------------------------------------
def _normal_loop(v, tri):
    """step 1 for one triangle -> three numpy float64 scalars, or None"""
    c = [[D(v[tri[k], a]) for a in range(3)] for k in range(3)]
    if not all(np.isfinite(x) for row in c for x in row):
        return None
    ab = [c[1][a] - c[0][a] for a in range(3)]
    ac = [c[2][a] - c[0][a] for a in range(3)]
    m = [ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]]
    l2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
    if not (l2 > 0 and np.isfinite(l2)):
        return None
    l = np.sqrt(l2)
    return [m[0] / l, m[1] / l, m[2] / l]


def _point_loop(tg, q, i, p, reach, huber):
    """steps 5 and 6 for one point -> the 28 terms, or None when the point is not used"""
    tri = int(q["triangle"][i])
    if tri == NONE or not q["distance"][i] <= F(reach):
        return None
    n = _normal_loop(tg.v, tg.t[tri])
    if n is None:
        return None
    P = [D(p[i, a]) for a in range(3)]
    e = [P[a] - D(q["closest"][i, a]) for a in range(3)]
    f = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
    J = n + [P[1] * n[2] - P[2] * n[1], P[2] * n[0] - P[0] * n[2], P[0] * n[1] - P[1] * n[0]]
    h = D(F(huber))
    w = D(1) if abs(f) <= h else h / abs(f)
    a = [w * j for j in J]
    return [float(a[i_] * J[j_]) for i_, j_ in PAIRS] + [float(a[i_] * f) for i_ in range(6)] + [float((w * f) * f)]


def system_loop(tg, pts, pose, stride, reach, huber):
    m = [D(x) for x in pose]
    n = len(pts)
    n_l = (n + stride - 1) // stride
    p = np.zeros((n_l, 3), F)
    with np.errstate(all="ignore"):
        for j in range(n_l):
            x = [D(pts[j * stride, a]) for a in range(3)]
            for k in range(3):
                p[j, k] = F(((m[3 * k] * x[0] + m[3 * k + 1] * x[1]) + m[3 * k + 2] * x[2]) + m[9 + k])
        q = tg.query_loop(p)
        used, groups = 0, []
        for g in range(max((n_l + 63) // 64, 1)):
            lanes = [[0.0] * 64 for _ in range(TERMS)]
            for lane in range(64):
                j = g * 64 + lane
                if j >= n_l:
                    continue
                tm = _point_loop(tg, q, j, p, reach, huber)
                if tm is None:
                    continue
                used += 1
                for k in range(TERMS):
                    lanes[k][lane] = tm[k]
            groups.append([AM.tree64_loop(lanes[k]) for k in range(TERMS)])
        return used, np.array([AM.reduce_loop([g[k] for g in groups]) for k in range(TERMS)], D)


def align_loop(tg, points, R, t, levels=None, huber=None, damping=0.0, eps=1e-7, min_points=6):
    R = np.asarray(R, D).reshape(-1, 3, 3); t = np.asarray(t, D).reshape(-1, 3)
    huber = tg.d_max if huber is None else huber
    pts = np.asarray(points, F).reshape(-1, 3)
    fn = lambda pose, stride, reach: system_loop(tg, pts, pose, stride, reach, huber)
    return _run(fn, R, t, levels_of(levels, tg.d_max), damping, eps, min_points)


# ---- the scenes of the tests ---------------------------------------------------------------------------------------------------------------
def surface(x, y, asymmetric=False):
    """section 18's surface; with `asymmetric` the terms that take away its half-turn symmetry"""
    z = 1.8 + 0.25 * np.sin(1.3 * x) * np.cos(0.9 * y) + 0.1 * x
    return z + 0.06 * x * x + 0.05 * y if asymmetric else z


def height_field(nx=33, ny=25, hx=1.6, hy=1.2, asymmetric=False):
    """the surface as a mesh of nx x ny vertices over +-hx x +-hy -> (vertices float32 [nx ny, 3], triangles int64 [2 (nx - 1)(ny - 1), 3])"""
    x, y = np.meshgrid(np.linspace(-hx, hx, nx), np.linspace(-hy, hy, ny))
    v = np.stack([x, y, surface(x, y, asymmetric)], -1).reshape(-1, 3).astype(F)
    i = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)[None]).reshape(-1)
    t = np.concatenate([np.stack([i, i + 1, i + nx + 1], 1), np.stack([i, i + nx + 1, i + nx], 1)])
    return v, t.astype(np.int64)


def surface_points(n=600, seed=3, hx=1.3, hy=0.95, asymmetric=False):
    """n analytic points of the surface inside +-hx x +-hy, float64 [n, 3]"""
    r = np.random.default_rng(seed)
    x, y = r.uniform(-hx, hx, n), r.uniform(-hy, hy, n)
    return np.stack([x, y, surface(x, y, asymmetric)], 1)


def rotation(axis, angle):
    """Rodrigues' formula, float64 [3, 3]"""
    a = np.asarray(axis, D) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], D)
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def perturbation(seed, angle, shift, centre=(0.0, 0.0, 1.8)):
    """a rigid motion of `angle` rad about a random axis through `centre` and `shift` m in a random direction -> (R, t)"""
    r = np.random.default_rng(seed)
    R = rotation(r.normal(size=3), angle)
    d = r.normal(size=3)
    c = np.asarray(centre, D)
    return R, c - R @ c + shift * d / np.linalg.norm(d)


def principal_starts(points, vertices):
    """rgbid.meshreg.principal_starts in numpy: the four proper rotations that map the source's principal axes onto the target's, the
    centroids matched -> (R [4, 3, 3], t [4, 3])"""
    def frame(x):
        x = np.asarray(x, D).reshape(-1, 3)
        x = x[np.isfinite(x).all(1)]
        c = x.mean(0)
        _, E = np.linalg.eigh((x - c).T @ (x - c) / len(x))
        if np.linalg.det(E) < 0:
            E = E * np.array([1.0, 1.0, -1.0])
        return c, E
    cs, Es = frame(points)
    ct, Et = frame(vertices)
    R = np.stack([Et @ np.diag(s) @ Es.T for s in ((1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))])
    return R, np.stack([ct - r @ cs for r in R])


def pose_error(R, t, R0=None, t0=None):
    """the angle (rad) and the distance (m) of the pose from (R0, t0), the identity by default"""
    R0 = np.eye(3) if R0 is None else np.asarray(R0, D)
    t0 = np.zeros(3) if t0 is None else np.asarray(t0, D)
    return AM.correction(R0, t0, np.asarray(R, D).reshape(3, 3), np.asarray(t, D))
