"""numpy restatement of the rasteriser's contract (include/rgbid_raster.h), steps 3 - 9, stated twice: vectorised
over (triangle, pixel) pairs in int64 / float64 arrays with np.minimum.at for the winner, and as plain scalar loops over Python integers
and floats (`*_loop`).  Both are written from the contract, not from the kernels.  Integers decide coverage and the winner; float32
operations are numpy float32 scalars or arrays (one rounding per operation), doubles are Python / numpy doubles."""
import math

import numpy as np

from tests.render_mirror import pose_cw

F, U32, U64 = np.float32, np.uint32, np.uint64
EMPTY = U32(0xFFFFFFFF)
NAN_BITS = U32(0x7FFFFFFF)
EMPTY_KEY = U64(0xFFFFFFFFFFFFFFFF)
SUB = 256
MAX_DIM = 16384
GUARD = float(1 << 23)
COUNTS = ("gated", "degenerate", "empty_box", "drawn", "fragments", "pixels")
PAIR_BATCH = 1 << 21                     # (triangle, pixel) pairs the vectorised statement expands at a time


def _mesh(vertices, triangles):
    pos = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    tri = np.ascontiguousarray(np.asarray(triangles).reshape(-1, 3)).astype(np.int64) & 0xFFFFFFFF
    if len(tri) and tri.max() >= len(pos):
        raise ValueError("a triangle names a vertex that does not exist")      # step 1: the mesh is refused
    return pos, tri


# ---- the vectorised statement -----------------------------------------------------------------------------------------------------------
def project(pos, m, K, z_min, z_max):
    """step 3 for one view: -> (xs, ys int64, Z float32, usable bool) per vertex; xs, ys are 0 where the vertex is not usable"""
    fx, fy, cx, cy = (F(v) for v in K)
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    with np.errstate(all="ignore"):
        X = ((m[0] * x + m[1] * y) + m[2] * z) + m[9]
        Y = ((m[3] * x + m[4] * y) + m[5] * z) + m[10]
        Z = ((m[6] * x + m[7] * y) + m[8] * z) + m[11]
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (Z >= F(z_min)) & (Z <= F(z_max))
        u = fx * (X / Z) + cx
        v = fy * (Y / Z) + cy
        xs = np.floor(u * F(256) + F(0.5))
        ys = np.floor(v * F(256) + F(0.5))
        ok &= (np.abs(xs) <= F(GUARD)) & (np.abs(ys) <= F(GUARD))          # NaN and infinity fail
    assert X.dtype == F and xs.dtype == F
    return np.where(ok, xs, 0).astype(np.int64), np.where(ok, ys, 0).astype(np.int64), Z.astype(F), ok


def classify(tri, xs, ys, ok, rows, cols):
    """step 4 -> dict(cls int [n_t]: 0 gated, 1 degenerate, 2 empty box, 3 drawn; A, x0, x1, y0, y1 int64)"""
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    usable = ok[a] & ok[b] & ok[c]
    A = (xs[b] - xs[a]) * (ys[c] - ys[a]) - (ys[b] - ys[a]) * (xs[c] - xs[a])
    tx, ty = np.stack([xs[a], xs[b], xs[c]]), np.stack([ys[a], ys[b], ys[c]])
    x0 = np.maximum(0, -((-tx.min(0)) // SUB)); x1 = np.minimum(cols - 1, tx.max(0) // SUB)      # // floors towards -inf
    y0 = np.maximum(0, -((-ty.min(0)) // SUB)); y1 = np.minimum(rows - 1, ty.max(0) // SUB)
    cls = np.full(len(tri), 3)
    cls[(x0 > x1) | (y0 > y1)] = 2
    cls[A == 0] = 1
    cls[~usable] = 0
    return dict(cls=cls, A=A, x0=x0, x1=x1, y0=y0, y1=y1)


def edges(tri_rows, xs, ys, A, px, py):
    """step 5 for pairs (triangle row [3 indices], pixel) -> Ea, Eb, Ec int64"""
    a, b, c = tri_rows[:, 0], tri_rows[:, 1], tri_rows[:, 2]
    s = np.sign(A)
    Px, Py = SUB * px, SUB * py
    Ea = s * ((xs[c] - xs[b]) * (Py - ys[b]) - (ys[c] - ys[b]) * (Px - xs[b]))
    Eb = s * ((xs[a] - xs[c]) * (Py - ys[c]) - (ys[a] - ys[c]) * (Px - xs[c]))
    Ec = s * ((xs[b] - xs[a]) * (Py - ys[a]) - (ys[b] - ys[a]) * (Px - xs[a]))
    return Ea, Eb, Ec


def weights(tri_rows, Z, Ea, Eb, Ec):
    """step 6 -> pa, pb, pc, q in double"""
    with np.errstate(all="ignore"):      # a vertex that is not usable has any Z; no pair reads it
        w = 1.0 / Z.astype(np.float64)
    pa, pb, pc = Ea.astype(np.float64) * w[tri_rows[:, 0]], Eb.astype(np.float64) * w[tri_rows[:, 1]], Ec.astype(np.float64) * w[tri_rows[:, 2]]
    return pa, pb, pc, (pa + pb) + pc


def view_keys(pos, tri, m, K, rows, cols, z_min, z_max):
    """steps 3 - 7 for one view -> (keys uint64 [rows, cols], counts[:5], projection, classes)"""
    xs, ys, Z, ok = project(pos, m, K, z_min, z_max)
    cl = classify(tri, xs, ys, ok, rows, cols)
    keys = np.full(rows * cols, EMPTY_KEY, U64)
    drawn = np.flatnonzero(cl["cls"] == 3)
    w = cl["x1"][drawn] - cl["x0"][drawn] + 1
    size = w * (cl["y1"][drawn] - cl["y0"][drawn] + 1)
    fragments, lo = 0, 0
    while lo < len(drawn):
        hi = lo + max(1, int(np.searchsorted(np.cumsum(size[lo:]), PAIR_BATCH, "right")))
        t = np.repeat(drawn[lo:hi], size[lo:hi])
        k = np.arange(len(t)) - np.repeat(np.cumsum(size[lo:hi]) - size[lo:hi], size[lo:hi])
        wt = np.repeat(w[lo:hi], size[lo:hi])
        px, py = cl["x0"][t] + k % wt, cl["y0"][t] + k // wt
        Ea, Eb, Ec = edges(tri[t], xs, ys, cl["A"][t], px, py)
        assert (Ea + Eb + Ec == np.abs(cl["A"][t])).all()
        cov = (Ea >= 0) & (Eb >= 0) & (Ec >= 0)
        t, px, py = t[cov], px[cov], py[cov]
        _, _, _, q = weights(tri[t], Z, Ea[cov], Eb[cov], Ec[cov])
        Zp = (np.abs(cl["A"][t]).astype(np.float64) / q).astype(F)
        assert (q > 0).all() and (Zp > 0).all()
        np.minimum.at(keys, py * cols + px, (Zp.view(U32).astype(U64) << U64(32)) | t.astype(U64))
        fragments += int(cov.sum())
        lo = hi
    counts = [int((cl["cls"] == k).sum()) for k in range(4)] + [fragments]
    return keys.reshape(rows, cols), counts, (xs, ys, Z, ok), cl


def resolve(keys, tri, proj, cl, m, colours=None, normals=None):
    """step 8 -> dict(index uint32, depth float32 [rows, cols], colour uint8 [rows, cols, 3], normal float32 [3, rows, cols]); the
    attribute planes only with their attributes"""
    rows, cols = keys.shape
    xs, ys, Z, _ = proj
    won = keys != EMPTY_KEY
    out = dict(index=np.where(won, keys & U64(0xFFFFFFFF), U64(EMPTY)).astype(U32),
               depth=np.where(won, (keys >> U64(32)).astype(U32), NAN_BITS).astype(U32).view(F))
    py, px = np.nonzero(won)
    t = out["index"][py, px].astype(np.int64)
    Ea, Eb, Ec = edges(tri[t], xs, ys, cl["A"][t], px, py)
    pa, pb, pc, q = weights(tri[t], Z, Ea, Eb, Ec)
    if colours is not None:
        col = np.ascontiguousarray(colours, np.uint8).reshape(-1, 3).astype(np.float64)
        plane = np.zeros((rows, cols, 3), np.uint8)
        for k in range(3):
            f = np.floor(((pa * col[tri[t, 0], k] + pb * col[tri[t, 1], k]) + pc * col[tri[t, 2], k]) / q + 0.5)
            plane[py, px, k] = np.clip(f, 0, 255).astype(np.uint8)
        out["colour"] = plane
    if normals is not None:
        nr = np.ascontiguousarray(normals, F).reshape(-1, 3).astype(np.float64)
        r = m.astype(np.float64)
        plane = np.full((3, rows, cols), NAN_BITS, U32).view(F)
        with np.errstate(all="ignore"):
            mk = [(pa * nr[tri[t, 0], k] + pb * nr[tri[t, 1], k]) + pc * nr[tri[t, 2], k] for k in range(3)]
            c = [(r[3 * k] * mk[0] + r[3 * k + 1] * mk[1]) + r[3 * k + 2] * mk[2] for k in range(3)]
            g = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
            good = (g != 0) & np.isfinite(g)
            for k in range(3):
                plane[k, py, px] = np.where(good, c[k] / np.sqrt(g), 0.0).astype(F)
        out["normal"] = plane
    return out


def raster_numpy(vertices, triangles, R, t, K, rows, cols, colours=None, normals=None, z_min=0.05, z_max=20.0):
    """the mesh seen from the world poses R [V, 3, 3], t [V, 3] -> dict of index uint32 [V, rows, cols], depth float32 [V, rows, cols],
    colour uint8 [V, rows, cols, 3] (with colours), normal float32 [V, 3, rows, cols] (with normals), counts int64 [V, 6]"""
    pos, tri = _mesh(vertices, triangles)
    R = np.asarray(R, np.float64).reshape(-1, 3, 3); t = np.asarray(t, np.float64).reshape(-1, 3)
    planes, counts = [], []
    for v in range(len(R)):
        m = pose_cw(R[v], t[v])
        keys, cnt, proj, cl = view_keys(pos, tri, m, K, rows, cols, z_min, z_max)
        planes.append(resolve(keys, tri, proj, cl, m, colours, normals))
        counts.append(cnt + [int((keys != EMPTY_KEY).sum())])
    out = {k: np.stack([p[k] for p in planes]) for k in planes[0]}
    out["counts"] = np.array(counts, np.int64)
    return out


# ---- the scalar statement ---------------------------------------------------------------------------------------------------------------
def _fin(x):
    return math.isfinite(float(x))


def project_loop(p, m, K, z_min, z_max):
    """step 3 for one vertex p (three float32) -> (xs, ys, Z) with Python integers and a float32 Z, or None when it is not usable"""
    fx, fy, cx, cy = (F(v) for v in K)
    x, y, z = (F(v) for v in p)
    if not (_fin(x) and _fin(y) and _fin(z)):
        return None
    with np.errstate(all="ignore"):
        X = F(F(F(m[0] * x) + F(m[1] * y)) + F(m[2] * z)) + m[9]
        Y = F(F(F(m[3] * x) + F(m[4] * y)) + F(m[5] * z)) + m[10]
        Z = F(F(F(m[6] * x) + F(m[7] * y)) + F(m[8] * z)) + m[11]
        if not (Z >= F(z_min) and Z <= F(z_max)):
            return None
        u = F(fx * F(X / Z)) + cx
        v = F(fy * F(Y / Z)) + cy
        us, vs = F(F(u * F(256)) + F(0.5)), F(F(v * F(256)) + F(0.5))
    if not (_fin(us) and _fin(vs)):
        return None
    xs, ys = math.floor(float(us)), math.floor(float(vs))
    if abs(xs) > 1 << 23 or abs(ys) > 1 << 23:
        return None
    return xs, ys, F(Z)


def _floor_div(a, b):
    return a // b                        # Python's // floors towards -inf


def _ceil_div(a, b):
    return -((-a) // b)


def _edges_loop(a, b, c, s, px, py):
    Px, Py = SUB * px, SUB * py
    return (s * ((c[0] - b[0]) * (Py - b[1]) - (c[1] - b[1]) * (Px - b[0])), s * ((a[0] - c[0]) * (Py - c[1]) - (a[1] - c[1]) * (Px - c[0])),
            s * ((b[0] - a[0]) * (Py - a[1]) - (b[1] - a[1]) * (Px - a[0])))


def _weights_loop(a, b, c, E):
    pa, pb, pc = float(E[0]) * (1.0 / float(a[2])), float(E[1]) * (1.0 / float(b[2])), float(E[2]) * (1.0 / float(c[2]))
    return pa, pb, pc, (pa + pb) + pc


def raster_loop(vertices, triangles, R, t, K, rows, cols, colours=None, normals=None, z_min=0.05, z_max=20.0):
    """raster_numpy as scalar loops: per view a dictionary pixel -> (bits of Zp, triangle) minimum"""
    pos, tri = _mesh(vertices, triangles)
    R = np.asarray(R, np.float64).reshape(-1, 3, 3); t = np.asarray(t, np.float64).reshape(-1, 3)
    V = len(R)
    out = dict(index=np.full((V, rows, cols), EMPTY, U32), depth=np.full((V, rows, cols), NAN_BITS, U32).view(F), counts=np.zeros((V, 6), np.int64))
    if colours is not None:
        out["colour"] = np.zeros((V, rows, cols, 3), np.uint8)
    if normals is not None:
        out["normal"] = np.full((V, 3, rows, cols), NAN_BITS, U32).view(F)
    for v in range(V):
        m = pose_cw(R[v], t[v])
        rec = [project_loop(p, m, K, z_min, z_max) for p in pos]
        best, setup, cnt = {}, {}, out["counts"][v]
        for ti, (ia, ib, ic) in enumerate(tri.tolist()):
            a, b, c = rec[ia], rec[ib], rec[ic]
            if a is None or b is None or c is None:
                cnt[0] += 1; continue
            A = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
            if A == 0:
                cnt[1] += 1; continue
            x0, x1 = max(0, _ceil_div(min(a[0], b[0], c[0]), SUB)), min(cols - 1, _floor_div(max(a[0], b[0], c[0]), SUB))
            y0, y1 = max(0, _ceil_div(min(a[1], b[1], c[1]), SUB)), min(rows - 1, _floor_div(max(a[1], b[1], c[1]), SUB))
            if x0 > x1 or y0 > y1:
                cnt[2] += 1; continue
            cnt[3] += 1
            s = 1 if A > 0 else -1
            setup[ti] = (a, b, c, s)
            for py in range(y0, y1 + 1):
                for px in range(x0, x1 + 1):
                    E = _edges_loop(a, b, c, s, px, py)
                    assert sum(E) == abs(A) and max(abs(e) for e in E) < 1 << 49
                    if E[0] < 0 or E[1] < 0 or E[2] < 0:
                        continue
                    cnt[4] += 1
                    q = _weights_loop(a, b, c, E)[3]
                    Zp = F(float(abs(A)) / q)
                    assert q > 0 and Zp > 0
                    key = (int(np.array(Zp, F).view(U32)), ti)
                    if (px, py) not in best or key < best[(px, py)]:
                        best[(px, py)] = key
        cnt[5] = len(best)
        for (px, py), (bits, ti) in best.items():
            out["index"][v, py, px] = ti
            out["depth"].view(U32)[v, py, px] = bits
            a, b, c, s = setup[ti]
            pa, pb, pc, q = _weights_loop(a, b, c, _edges_loop(a, b, c, s, px, py))
            ia, ib, ic = tri[ti]
            if colours is not None:
                for k in range(3):
                    f = math.floor(((pa * float(colours[ia][k]) + pb * float(colours[ib][k])) + pc * float(colours[ic][k])) / q + 0.5)
                    out["colour"][v, py, px, k] = min(255, max(0, f))
            if normals is not None:
                mk = [(pa * float(normals[ia][k]) + pb * float(normals[ib][k])) + pc * float(normals[ic][k]) for k in range(3)]
                cw = [(float(m[3 * k]) * mk[0] + float(m[3 * k + 1]) * mk[1]) + float(m[3 * k + 2]) * mk[2] for k in range(3)]
                g = (cw[0] * cw[0] + cw[1] * cw[1]) + cw[2] * cw[2]
                for k in range(3):
                    out["normal"][v, k, py, px] = F(cw[k] / math.sqrt(g)) if g != 0 and math.isfinite(g) else F(0)
    return out


def same(a, b, keys=None):
    """whether two results agree byte for byte on the given keys (all of a's by default)"""
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() and np.asarray(a[k]).shape == np.asarray(b[k]).shape
               for k in (keys or a.keys()))
