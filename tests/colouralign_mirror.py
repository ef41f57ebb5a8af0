"""numpy restatement of the colour alignment contract (include/rgbid_colouralign.h): the judge of
csrc/kernels_colouralign.hip.  Step 3 is tests/recolour_mirror.py's view_pairs, the tree, the solve and the update are
tests/align_mirror.py's, the grouping of the lattice is tests/meshreg_mirror.py's; every double is formed by float64 operations in exactly
the order of the header, integers and comparisons decide.  `run` is vectorised over the lattice of one view; `pair_loop` is the plain
scalar restatement of one pair that the CPU tests hold it against."""
import math

import numpy as np

from tests import align_mirror as AM
from tests import meshreg_mirror as MR
from tests import raster_mirror as XM
from tests import recolour_mirror as RM
from tests.render_mirror import pose_cw

F, D, U8, U32, U64, I64 = np.float32, np.float64, np.uint8, np.uint32, np.uint64, np.int64
RUNNING, CONVERGED, FEW, SINGULAR, FIXED = 0, 1, 2, 3, 4
STATUS_NAMES = ("running", "converged", "few", "singular", "fixed")
TERMS, PAIRS = AM.TERMS, AM.PAIRS
RESULT_DTYPE = AM.RESULT_DTYPE                                    # rgbid_colouralign_result is laid out as rgbid_meshreg_result
MAX_VIEWS, MAX_ITERATIONS = 2048, 256
assert MAX_VIEWS * RM.UNIT * 65280 * 65536 < 1 << 53             # step 5: S is exact as a double
PARAMS = dict(z_min=0.05, z_max=20.0, surface_tolerance=0.02, measured_tolerance=0.02, min_cos=0.2, two_sided=False)
RULE = dict(huber=16.0, damping=0.0, eps=1e-7, min_pairs=6, min_views=2, rounds=4, iterations=3, stride=1)


def grey_plane(colour):
    """step 4: uint8 [rows, cols, 3] -> L = 77 R + 150 G + 29 B as int64 [rows cols]"""
    c = np.ascontiguousarray(colour, U8).reshape(-1, 3).astype(I64)
    return 77 * c[:, 0] + 150 * c[:, 1] + 29 * c[:, 2]


def grey_sample(L, tex, ax, ay):
    """step 4 for footprints tex [4, n] (00 10 01 11) and fractions ax, ay -> (s, Gx, Gy) as int64"""
    ax, ay = ax.astype(I64), ay.astype(I64)
    L00, L10, L01, L11 = (L[tex[k]] for k in range(4))
    s = (256 - ax) * (256 - ay) * L00 + ax * (256 - ay) * L10 + (256 - ax) * ay * L01 + ax * ay * L11
    Gx = (256 - ay) * (L10 - L00) + ay * (L11 - L01)
    Gy = (256 - ax) * (L01 - L00) + ax * (L11 - L10)
    assert not s.size or (0 <= int(s.min()) and int(s.max()) <= 65280 * 65536)
    return s, Gx, Gy


def pair_values(pos, nrm, m, K, rows, cols, colour, surface, measured, prm):
    """steps 3 and 4 of one view at the twelve floats m over the lattice's vertices -> dict(cls int [n_l], taken: indices of the TAKEN
    vertices, and of those w uint64, s, Gx, Gy int64, X, Y, Z float32, xs, ys: the snapped positions)"""
    cls, taken, w, _ = RM.view_pairs(pos, nrm, m, K, rows, cols, colour, surface, measured, prm["z_min"], prm["z_max"], prm["surface_tolerance"],
                                     prm["measured_tolerance"], prm["min_cos"], prm["two_sided"])
    xs, ys, Z, ok = XM.project(pos, m, K, prm["z_min"], prm["z_max"])
    assert ok[taken].all()
    tex, ax, ay = RM.footprint(xs[taken], ys[taken], rows, cols)
    s, Gx, Gy = grey_sample(grey_plane(colour), tex.astype(I64), ax, ay)
    p = pos[taken]
    with np.errstate(all="ignore"):
        X = ((m[0] * p[:, 0] + m[1] * p[:, 1]) + m[2] * p[:, 2]) + m[9]
        Y = ((m[3] * p[:, 0] + m[4] * p[:, 1]) + m[5] * p[:, 2]) + m[10]
    assert X.dtype == F and Y.dtype == F
    return dict(cls=cls, taken=taken, w=w, s=s, Gx=Gx, Gy=Gy, X=X, Y=Y, Z=Z[taken], xs=xs[taken], ys=ys[taken])


def jacobian(pv, pos, m, K):
    """step 6's J for the TAKEN pairs of pair_values -> list of 6 float64 arrays"""
    fx, fy = D(F(K[0])), D(F(K[1]))
    r = m.astype(D)
    with np.errstate(all="ignore"):
        dx, dy = pv["Gx"].astype(D) / 65536.0, pv["Gy"].astype(D) / 65536.0
        X, Y, Z = pv["X"].astype(D), pv["Y"].astype(D), pv["Z"].astype(D)
        iz = 1.0 / Z
        a, b = (dx * fx) * iz, (dy * fy) * iz
        c = -((a * X + b * Y) * iz)
        mm = [(r[i] * a + r[3 + i] * b) + r[6 + i] * c for i in range(3)]
        p = pos[pv["taken"]].astype(D)
        p0, p1, p2 = p[:, 0], p[:, 1], p[:, 2]
        return [-mm[0], -mm[1], -mm[2], -(p1 * mm[2] - p2 * mm[1]), -(p2 * mm[0] - p0 * mm[2]), -(p0 * mm[1] - p1 * mm[0])]


def lattice(vertices, normals, stride):
    pos = np.ascontiguousarray(vertices, F).reshape(-1, 3)[::stride]
    nrm = None if normals is None else np.ascontiguousarray(normals, F).reshape(-1, 3)[::stride]
    return pos, nrm


def targets(pos, nrm, ms, K, rows, cols, colours, surface, measured, prm):
    """step 5 over the lattice at the views' twelve floats ms -> (S uint64, W uint64, used uint32) [n_l]"""
    S, W, used = np.zeros(len(pos), U64), np.zeros(len(pos), U64), np.zeros(len(pos), U32)
    for v, m in enumerate(ms):
        pv = pair_values(pos, nrm, m, K, rows, cols, colours[v], None if surface is None else surface[v],
                         None if measured is None else measured[v], prm)
        S[pv["taken"]] += pv["w"] * pv["s"].astype(U64)
        W[pv["taken"]] += pv["w"]
        used[pv["taken"]] += U32(1)
    assert not S.size or int(S.max()) < 1 << 53
    return S, W, used


def target_values(S, W, used, min_views):
    """step 5 -> (has bool, C float64: NaN-free only where has)"""
    with np.errstate(all="ignore"):
        return used >= min_views, S.astype(D) / (W.astype(D) * 16777216.0)


def terms(pos, nrm, m, K, rows, cols, colour, surface, measured, prm, has, C, huber):
    """step 6's terms of one view -> (used bool [n_l], float64 [28, n_l], +0.0 where the pair is not used)"""
    pv = pair_values(pos, nrm, m, K, rows, cols, colour, surface, measured, prm)
    idx = pv["taken"]
    J = jacobian(pv, pos, m, K)
    with np.errstate(all="ignore"):
        f = pv["s"].astype(D) / 16777216.0 - C[idx]
        h = D(F(huber))
        wh = np.where(np.abs(f) <= h, D(1), h / np.abs(f))
        a = [wh * j for j in J]
        t = np.stack([a[i] * J[j] for i, j in PAIRS] + [a[i] * f for i in range(6)] + [(wh * f) * f])
    use = has[idx]
    out = np.zeros((TERMS, len(pos)), D)
    out[:, idx[use]] = t[:, use]
    used = np.zeros(len(pos), bool)
    used[idx[use]] = True
    return used, out


def system(*a):
    """step 6 for one view -> (used count, the 28 sums as float64, the used pairs per group of 64)"""
    used, t = terms(*a)
    return int(used.sum()), AM.reduce_tiles(AM.tree64(MR.group_lanes(t))), MR.group_lanes(used).sum(-1)


def check_rule(rule):
    r = dict(RULE, **rule)
    assert math.isfinite(float(F(r["huber"]))) and F(r["huber"]) > 0 and r["damping"] >= 0 and r["eps"] > 0 and r["min_pairs"] >= 6
    assert r["min_views"] >= 2 and r["rounds"] >= 1 and r["iterations"] >= 1 and r["rounds"] * r["iterations"] <= MAX_ITERATIONS and r["stride"] >= 1
    return r


def run(vertices, R, t, K, rows, cols, colours, surface=None, depthinv=None, normals=None, fixed=(), params=None, trace=None, **rule):
    """steps 1 - 8 -> dict(records RESULT_DTYPE [V] as the device writes them, S, W, used: the last round's targets).  fixed: the indices of
    the views whose pose is held.  trace: a list that receives (round, iteration, view, used pairs per group) of every system built"""
    rule, prm = check_rule(rule), dict(PARAMS, **(params or {}))
    R = np.asarray(R, D).reshape(-1, 3, 3); t = np.asarray(t, D).reshape(-1, 3)
    V = len(R)
    assert 1 <= V <= MAX_VIEWS and len(colours) == V
    pos, nrm = lattice(vertices, normals, rule["stride"])
    poses = [np.concatenate([R[v].reshape(9), t[v]]).astype(D) for v in range(V)]
    status = [FIXED if v in set(fixed) else RUNNING for v in range(V)]
    out = np.zeros(V, RESULT_DTYPE)
    its = [0] * V
    cw = lambda pose: pose_cw(pose[:9], pose[9:])
    S = W = used = None
    for rnd in range(rule["rounds"]):
        S, W, used = targets(pos, nrm, [cw(p) for p in poses], K, rows, cols, colours, surface, depthinv, prm)
        has, C = target_values(S, W, used, rule["min_views"])
        for v in range(V):
            if status[v] == CONVERGED:
                status[v] = RUNNING
            for it in range(rule["iterations"]):
                if status[v] != RUNNING:
                    break
                n_used, sums, per_group = system(pos, nrm, cw(poses[v]), K, rows, cols, colours[v], None if surface is None else surface[v],
                                                 None if depthinv is None else depthinv[v], prm, has, C, rule["huber"])
                if trace is not None:
                    trace.append((rnd, it, v, per_group))
                if its[v] == 0:
                    out[v]["used"][0], out[v]["sums"][0] = n_used, AM.one_nan(sums)
                out[v]["used"][1], out[v]["sums"][1] = n_used, AM.one_nan(sums)
                its[v] += 1
                if n_used < rule["min_pairs"]:
                    status[v] = FEW
                    break
                delta = AM.solve(sums, rule["damping"])
                if delta is None:
                    status[v] = SINGULAR
                    break
                poses[v] = AM.update(poses[v], delta)
                if max(abs(x) for x in delta) < rule["eps"]:
                    status[v] = CONVERGED
    for v in range(V):
        out[v]["pose"], out[v]["status"], out[v]["iterations"] = AM.one_nan(poses[v]), status[v], its[v]
    return dict(records=out, S=S, W=W, used=used)


as_dict = AM.as_dict


def cost_per_pair(records):
    """sums[.][27] / used[.] of the first and of the last system of every view, float64 [V, 2] (NaN without a used pair)"""
    with np.errstate(all="ignore"):
        return records["sums"][:, :, 27] / records["used"].astype(D)


# ---- the scalar restatement of one pair ---------------------------------------------------------------------------------------------------
def pair_loop(p, n, m, K, rows, cols, colour, surface, measured, prm):
    """steps 3 and 4 for one vertex p (three float32) with the normal n (or None) -> None unless TAKEN, else dict(w, s, Gx, Gy: Python
    integers; X, Y, Z float32)"""
    q = XM.project_loop(p, m, K, prm["z_min"], prm["z_max"])
    if q is None:
        return None
    xs, ys, Z = q
    if not (0 <= xs <= 256 * (cols - 1) and 0 <= ys <= 256 * (rows - 1)):
        return None
    x0, y0, ax, ay = xs >> 8, ys >> 8, xs & 255, ys & 255
    x1, y1 = min(x0 + 1, cols - 1), min(y0 + 1, rows - 1)
    foot = [(y0, x0), (y0, x1), (y1, x0), (y1, x1)]
    with np.errstate(all="ignore"):
        if surface is not None:
            for y, x in foot:
                d = F(surface[y, x])
                if not np.isfinite(d) or abs(F(Z - d)) > F(prm["surface_tolerance"]):
                    return None
        if measured is not None:
            for y, x in foot:
                iD = F(measured[y, x])
                if not (np.isfinite(iD) and iD > 0):
                    return None
                z = F(F(1) / iD)
                if not np.isfinite(z) or abs(F(Z - z)) > F(prm["measured_tolerance"]):
                    return None
        x, y, z = (F(v) for v in p)
        X = F(F(F(m[0] * x) + F(m[1] * y)) + F(m[2] * z)) + m[9]
        Y = F(F(F(m[3] * x) + F(m[4] * y)) + F(m[5] * z)) + m[10]
        w = RM.UNIT
        if n is not None:
            n0, n1, n2 = (F(v) for v in n)
            qq = F(F(F(n0 * n0) + F(n1 * n1)) + F(n2 * n2))
            if np.isfinite(qq) and qq != 0:
                c = [D(F(F(F(m[3 * k] * n0) + F(m[3 * k + 1] * n1)) + F(m[3 * k + 2] * n2))) for k in range(3)]
                Xd, Yd, Zd = D(X), D(Y), D(Z)
                dot = -((c[0] * Xd + c[1] * Yd) + c[2] * Zd)
                g = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
                r = (Xd * Xd + Yd * Yd) + Zd * Zd
                cos = dot / np.sqrt(g * r)
                if prm["two_sided"]:
                    cos = abs(cos)
                if not (cos > 0 and cos >= D(F(prm["min_cos"]))):
                    return None
                w = max(1, int(math.floor(float(cos) * 1024.0 + 0.5)))
    col = np.asarray(colour, U8)
    L = [77 * int(col[y, x, 0]) + 150 * int(col[y, x, 1]) + 29 * int(col[y, x, 2]) for y, x in foot]
    s = (256 - ax) * (256 - ay) * L[0] + ax * (256 - ay) * L[1] + (256 - ax) * ay * L[2] + ax * ay * L[3]
    Gx = (256 - ay) * (L[1] - L[0]) + ay * (L[3] - L[2])
    Gy = (256 - ax) * (L[2] - L[0]) + ax * (L[3] - L[1])
    return dict(w=w, s=s, Gx=Gx, Gy=Gy, X=F(X), Y=F(Y), Z=F(Z))


def terms_loop(pl, p, m, K, C, huber):
    """step 6 for one used pair (pl from pair_loop, the target C) -> the 28 terms as Python floats"""
    fx, fy = float(F(K[0])), float(F(K[1]))
    g, dx, dy = pl["s"] / 16777216.0, pl["Gx"] / 65536.0, pl["Gy"] / 65536.0
    f = g - float(C)
    X, Y, Z = float(pl["X"]), float(pl["Y"]), float(pl["Z"])
    iz = 1.0 / Z
    a, b = (dx * fx) * iz, (dy * fy) * iz
    c = -((a * X + b * Y) * iz)
    r = [float(x) for x in m]
    mm = [(r[i] * a + r[3 + i] * b) + r[6 + i] * c for i in range(3)]
    q = [float(F(x)) for x in p]
    J = [-mm[0], -mm[1], -mm[2], -(q[1] * mm[2] - q[2] * mm[1]), -(q[2] * mm[0] - q[0] * mm[2]), -(q[0] * mm[1] - q[1] * mm[0])]
    h = float(F(huber))
    wh = 1.0 if abs(f) <= h else h / abs(f)
    aa = [wh * j for j in J]
    return [aa[i] * J[j] for i, j in PAIRS] + [aa[i] * f for i in range(6)] + [(wh * f) * f]


# ---- the scale convention of rgbid.colouralign.refine_keyframes -----------------------------------------------------------------------------
def scaled_intrinsics(K, f):
    """K at 1 / f of the resolution, a pixel's centre at u = p: (fx / f, fy / f, (cx - (f - 1) / 2) / f, (cy - (f - 1) / 2) / f)"""
    fx, fy, cx, cy = (float(x) for x in K)
    return fx / f, fy / f, (cx - (f - 1) / 2.0) / f, (cy - (f - 1) / 2.0) / f


def box_filter(colour, f):
    """uint8 [rows, cols, 3] -> [rows // f, cols // f, 3]: (2 sum + f f) // (2 f f) per channel over the f x f boxes of the cropped plane"""
    c = np.ascontiguousarray(colour, U8)
    rows, cols = c.shape[0] // f, c.shape[1] // f
    s = c[:rows * f, :cols * f].astype(I64).reshape(rows, f, cols, f, 3).sum((1, 3))
    return ((2 * s + f * f) // (2 * f * f)).astype(U8)


def refine(vertices, R, t, K, rows, cols, colours, scales=(4, 2, 1), surface_of=None, **kw):
    """rgbid.colouralign.refine_keyframes' schedule: per scale f the box-filtered planes, the scaled intrinsics and one `run` that hands
    its poses on -> (R, t, the runs' results).  surface_of(R, t, K_f, rows_f, cols_f) gives the scale's surface planes, or None"""
    R = np.asarray(R, D).reshape(-1, 3, 3).copy(); t = np.asarray(t, D).reshape(-1, 3).copy()
    outs = []
    for f in scales:
        K_f, r_f, c_f = tuple(float(F(x)) for x in scaled_intrinsics(tuple(float(F(x)) for x in K), f)), rows // f, cols // f
        planes = [box_filter(c, f) for c in colours]
        out = run(vertices, R, t, K_f, r_f, c_f, planes, surface=None if surface_of is None else surface_of(R, t, K_f, r_f, c_f), **kw)
        R, t = out["records"]["pose"][:, :9].reshape(-1, 3, 3).copy(), out["records"]["pose"][:, 9:].copy()
        outs.append(out)
    return R, t, outs


# ---- the scene of the tests: a textured plane seen by a ring of cameras ----------------------------------------------------------------------
def texture(x, y):
    """a smooth grey pattern over the plane z = 0, 0 .. 255 as float64"""
    return 127.5 + 50.0 * np.sin(3.1 * x + 0.4) * np.cos(2.3 * y) + 40.0 * np.sin(1.7 * x * y + 0.9) + 30.0 * np.cos(5.3 * x - 4.1 * y)


def plane_vertices(nx=70, ny=55, hx=1.0, hy=0.75):
    """nx ny vertices of the plane z = 0 over +-hx x +-hy, float32 [nx ny, 3]"""
    x, y = np.meshgrid(np.linspace(-hx, hx, nx), np.linspace(-hy, hy, ny))
    return np.stack([x, y, np.zeros_like(x)], -1).reshape(-1, 3).astype(F)


def plane_triangles(nx=70, ny=55):
    """the triangles of plane_vertices' grid, facing the cameras of `ring`, int64 [2 (nx - 1)(ny - 1), 3]"""
    i = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)[None]).reshape(-1)
    return np.concatenate([np.stack([i, i + 1, i + nx + 1], 1), np.stack([i, i + nx + 1, i + nx], 1)]).astype(I64)


def look_at(eye, target=(0.0, 0.0, 0.0)):
    """the world pose R_WC, t_WC of a camera at `eye` that looks at `target`, its x axis horizontal"""
    eye, target = np.asarray(eye, D), np.asarray(target, D)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, np.array([0.0, -1.0, 0.0]))
    if np.linalg.norm(x) < 1e-9:
        x = np.array([1.0, 0.0, 0.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z], 1), eye


def render_plane(R, t, K, rows, cols):
    """the camera's image of the textured plane z = 0 -> uint8 [rows, cols, 3] (grey in all channels), by intersecting every pixel's ray"""
    fx, fy, cx, cy = (float(v) for v in K)
    u, v = np.meshgrid(np.arange(cols, dtype=D), np.arange(rows, dtype=D))
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ np.asarray(R, D).T
    with np.errstate(all="ignore"):
        lam = -t[2] / d[..., 2]
    x, y = t[0] + lam * d[..., 0], t[1] + lam * d[..., 1]
    g = np.clip(np.floor(texture(x, y) + 0.5), 0, 255)
    g = np.where(np.isfinite(g) & (lam > 0), g, 0).astype(U8)
    return np.repeat(g[..., None], 3, -1)


def ring(V=6, radius=0.35, height=1.6):
    """V camera poses on a circle above the plane, all looking at its centre -> (R [V, 3, 3], t [V, 3])"""
    poses = [look_at((radius * math.cos(2 * math.pi * k / V), radius * math.sin(2 * math.pi * k / V), -height)) for k in range(V)]
    return np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])


def perturb(R, t, size, seed):
    """the camera turned by `size` rad about a random axis through its centre and moved by `size` / 2 m in a random direction -> (R, t)"""
    r = np.random.default_rng(seed)
    dR = MR.rotation(r.normal(size=3), size)
    d = r.normal(size=3)
    return dR @ R, t + size * 0.5 * d / np.linalg.norm(d)


def pixel_error(vertices, K, Ra, ta, Rb, tb):
    """the mean distance in pixels between the projections of the vertices under the two world poses (float64)"""
    def proj(R, t):
        c = (np.asarray(vertices, D) - t) @ R
        return np.stack([K[0] * c[:, 0] / c[:, 2] + K[2], K[1] * c[:, 1] / c[:, 2] + K[3]], 1)
    return float(np.linalg.norm(proj(np.asarray(Ra, D), np.asarray(ta, D)) - proj(np.asarray(Rb, D), np.asarray(tb, D)), axis=1).mean())


def scene(V=6, rows=96, cols=128, size=0.006, seed=5, nx=70, ny=55):
    """the textured plane, its V true views and the poses perturbed by `size`, view 0 held -> dict"""
    K = (cols * 1.1, cols * 1.1, (cols - 1) / 2.0, (rows - 1) / 2.0)
    R, t = ring(V)
    colours = [render_plane(R[v], t[v], K, rows, cols) for v in range(V)]
    Rp, tp = R.copy(), t.copy()
    for v in range(1, V):
        Rp[v], tp[v] = perturb(R[v], t[v], size, seed + v)
    return dict(vertices=plane_vertices(nx, ny), K=K, rows=rows, cols=cols, R=R, t=t, Rp=Rp, tp=tp, colours=colours)
