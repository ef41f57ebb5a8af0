"""Numpy restatement of the point-to-mesh distance contract (include/rgbid_meshdist.h) that the GPU tests compare
the kernels against.  `query` is the brute force over all triangles: it prunes with step 3's box test, which is part of the contract,
evaluates step 4 only for the pairs that pass, every operation one float64 numpy call (so nothing is contracted), and lets step 5 decide.
`query_loop` is the same as plain scalar loops.  `plan` restates the grid (cell ranges, the runs in ascending triangle index, the pair
count and its refusal) and `candidates` what a query walks; `plan_loop` / `candidates_loop` do it with a dictionary of lists."""
import numpy as np

F, F64, U32 = np.float32, np.float64, np.uint32
NONE = 0xFFFFFFFF
NO_REGION = 255
NAN_BITS = 0x7FFFFFFF
MAX_CELL = 1 << 18
CELL_FACTOR = F(1.0625)
MIN_DISTANCE, MAX_DISTANCE = 2.0 ** -60, 2.0 ** 60
REGIONS = ("A", "B", "C", "AB", "AC", "BC", "face")


def prepare(vertices, triangles):
    """-> (vertices float32 [n_v, 3], triangles int64 [n_t, 3]); ValueError for an index that names no vertex"""
    v = np.ascontiguousarray(np.asarray(vertices, F).reshape(-1, 3))
    t = np.asarray(triangles)
    t = (t.view(U32) if t.dtype == np.int32 else t).astype(np.int64).reshape(-1, 3)
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("a triangle names a vertex that does not exist")
    return v, t


def distance32(d_max):
    d = F(d_max)
    if not (np.isfinite(d) and MIN_DISTANCE <= float(d) <= MAX_DISTANCE):
        raise ValueError("d_max must be finite and lie in [2^-60, 2^60]")
    return d


def corners(v, t):
    """-> (corners float32 [n_t, 3, 3], takes part bool [n_t], lo float32 [n_t, 3], hi float32 [n_t, 3])"""
    c = v[t] if len(t) else np.zeros((0, 3, 3), F)
    part = np.isfinite(c).all(axis=(1, 2))
    with np.errstate(invalid="ignore"):
        return c, part, c.min(axis=1), c.max(axis=1)


# ---- steps 3 - 5 ------------------------------------------------------------------------------------------------------------------------------
def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def closest_points(p, a, b, c):
    """step 4 for arrays of pairs, float64 [m, 3] each -> (r float64 [m, 3], region uint8 [m])"""
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        s, u = d4 - d3, d5 - d6
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (d6 >= 0) & (d5 <= d6), (vc <= 0) & (d1 >= 0) & (d3 <= 0),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (s >= 0) & (u >= 0)]
        region = np.select(conds, [0, 1, 2, 3, 4, 5], 6).astype(np.uint8)
        v_ab = (d1 / (d1 - d3))[:, None]
        w_ac = (d2 / (d2 - d6))[:, None]
        w_bc = (s / (s + u))[:, None]
        den = 1.0 / ((va + vb) + vc)
        v, w = (vb * den)[:, None], (vc * den)[:, None]
        cands = [a, b, c, a + v_ab * ab, a + w_ac * ac, b + w_bc * (c - b), (a + v * ab) + w * ac]
        r = np.select([(region == k)[:, None] for k in range(6)], cands[:6], cands[6])
    return r, region


def query(vertices, triangles, points, d_max, block=256):
    """steps 1 - 6 -> dict(triangle uint32 [n], distance float32 [n], closest float32 [n, 3], region uint8 [n], d2 float64 [n] (inf
    without a winner))"""
    v, t = prepare(vertices, triangles)
    q = np.ascontiguousarray(np.asarray(points, F).reshape(-1, 3))
    dm = F64(distance32(d_max))
    dm2 = dm * dm
    c, part, lo, hi = corners(v, t)
    tid = np.nonzero(part)[0]
    c64, lo64, hi64 = c[tid].astype(F64), lo[tid].astype(F64), hi[tid].astype(F64)
    n = len(q)
    best_t = np.full(n, NONE, np.int64)
    best_d2 = np.full(n, np.inf, F64)
    best_r = np.zeros((n, 3), F64)
    best_reg = np.full(n, NO_REGION, np.uint8)
    fin = np.isfinite(q).all(1)
    qs = np.nonzero(fin)[0]
    for b0 in range(0, len(qs), block):
        qi = qs[b0:b0 + block]
        q64 = q[qi].astype(F64)
        e = np.abs(q64[:, None, :] - np.minimum(np.maximum(q64[:, None, :], lo64[None]), hi64[None]))
        a_, b_ = np.nonzero((e <= dm).all(2))
        if not len(a_):
            continue
        p = q64[a_]
        r, region = closest_points(p, c64[b_, 0], c64[b_, 1], c64[b_, 2])
        with np.errstate(all="ignore"):
            ee = p - r
            d2 = (ee[:, 0] * ee[:, 0] + ee[:, 1] * ee[:, 1]) + ee[:, 2] * ee[:, 2]
            ok = ~np.isnan(d2) & (d2 <= dm2)
        a_, b_, r, region, d2 = a_[ok], b_[ok], r[ok], region[ok], d2[ok]
        if not len(a_):
            continue
        ti = tid[b_]
        order = np.lexsort((ti, d2, a_))
        first = order[np.r_[True, a_[order][1:] != a_[order][:-1]]]
        w = qi[a_[first]]
        best_t[w], best_d2[w], best_r[w], best_reg[w] = ti[first], d2[first], r[first], region[first]
    return _results(best_t, best_d2, best_r, best_reg)


def _results(best_t, best_d2, best_r, best_reg):
    won = best_t != NONE
    nan = np.array([NAN_BITS], U32).view(F)[0]
    dist = np.full(len(best_t), nan, F)
    dist[won] = np.sqrt(best_d2[won]).astype(F)
    closest = np.full((len(best_t), 3), nan, F)
    closest[won] = best_r[won].astype(F)
    return dict(triangle=best_t.astype(U32), distance=dist, closest=closest, region=best_reg.astype(np.uint8), d2=best_d2)


def closest_point_loop(p, a, b, c):
    """step 4 for one pair, numpy float64 scalars -> (r[3], region)"""
    sub = lambda x, y: [x[0] - y[0], x[1] - y[1], x[2] - y[2]]
    dot = lambda x, y: (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]
    ab, ac, ap, bp, cp = sub(b, a), sub(c, a), sub(p, a), sub(p, b), sub(p, c)
    d1, d2 = dot(ab, ap), dot(ac, ap)
    if d1 <= 0 and d2 <= 0:
        return list(a), 0
    d3, d4 = dot(ab, bp), dot(ac, bp)
    if d3 >= 0 and d4 <= d3:
        return list(b), 1
    d5, d6 = dot(ab, cp), dot(ac, cp)
    if d6 >= 0 and d5 <= d6:
        return list(c), 2
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        v = d1 / (d1 - d3)
        return [a[k] + v * ab[k] for k in range(3)], 3
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        w = d2 / (d2 - d6)
        return [a[k] + w * ac[k] for k in range(3)], 4
    va = d3 * d6 - d5 * d4
    s, u = d4 - d3, d5 - d6
    if va <= 0 and s >= 0 and u >= 0:
        w = s / (s + u)
        return [b[k] + w * (c[k] - b[k]) for k in range(3)], 5
    den = F64(1.0) / ((va + vb) + vc)
    v, w = vb * den, vc * den
    return [(a[k] + v * ab[k]) + w * ac[k] for k in range(3)], 6


def query_loop(vertices, triangles, points, d_max):
    """steps 1 - 6 as scalar loops over every (query, triangle) pair"""
    v, t = prepare(vertices, triangles)
    q = np.asarray(points, F).reshape(-1, 3)
    dm = F64(distance32(d_max))
    dm2 = dm * dm
    n = len(q)
    best_t = np.full(n, NONE, np.int64)
    best_d2 = np.full(n, np.inf, F64)
    best_r = np.zeros((n, 3), F64)
    best_reg = np.full(n, NO_REGION, np.uint8)
    tris = []
    for ti in range(len(t)):
        cs = [[F64(v[t[ti, k], a]) for a in range(3)] for k in range(3)]
        if all(np.isfinite(x) for row in cs for x in row):
            lo = [min(cs[0][a], cs[1][a], cs[2][a]) for a in range(3)]
            hi = [max(cs[0][a], cs[1][a], cs[2][a]) for a in range(3)]
            tris.append((ti, cs, lo, hi))
    with np.errstate(all="ignore"):
        for i in range(n):
            p = [F64(q[i, a]) for a in range(3)]
            if not all(np.isfinite(x) for x in p):
                continue
            for ti, cs, lo, hi in tris:
                if not all(abs(p[a] - min(max(p[a], lo[a]), hi[a])) <= dm for a in range(3)):
                    continue
                r, region = closest_point_loop(p, cs[0], cs[1], cs[2])
                e = [p[a] - r[a] for a in range(3)]
                d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
                if np.isnan(d2) or not d2 <= dm2:
                    continue
                if d2 < best_d2[i] or (d2 == best_d2[i] and ti < best_t[i]):
                    best_t[i], best_d2[i], best_r[i], best_reg[i] = ti, d2, r, region
    return _results(best_t, best_d2, best_r, best_reg)


def same(a, b, keys=("triangle", "distance", "closest", "region")):
    """the keys whose bytes differ"""
    return [k for k in keys if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


# ---- the grid ---------------------------------------------------------------------------------------------------------------------------------
def cell_size(d_max, cell=None):
    """the cell edge in float32: d_max * 1.0625f by default; ValueError for a smaller one"""
    least = distance32(d_max) * CELL_FACTOR
    if cell is None:
        return least
    c = F(cell)
    if not (np.isfinite(c) and c >= least and float(c) <= MAX_DISTANCE * 1.0625):
        raise ValueError("cell must be finite and at least 1.0625 d_max")
    return c


def _floor_cell(p, inv):
    """floorf(p * inv) in float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.floor(np.asarray(p, F) * inv)


def plan(vertices, triangles, d_max, cell=None, max_pairs=None):
    """the grid -> dict(grid int64 [6] = min_b, div_b; participating, pairs, cells, longest_run; inv, min_b, div; keys int64 [pairs] and
    tris int64 [pairs], sorted by key, a run in ascending triangle; ukeys, starts [cells + 1]).  ValueError when the box leaves
    |floorf(p inv)| <= 2^18 or the mesh needs more than max_pairs pairs (its .args[1] is the count)"""
    v, t = prepare(vertices, triangles)
    c = cell_size(d_max, cell)
    inv = F(1.0) / c
    _, part, lo, hi = corners(v, t)
    tid = np.nonzero(part)[0]
    out = dict(grid=np.zeros(6, np.int64), participating=len(tid), pairs=0, cells=0, longest_run=0, inv=inv, min_b=np.zeros(3, np.int64),
               div=np.zeros(3, np.int64), keys=np.zeros(0, np.int64), tris=np.zeros(0, np.int64), ukeys=np.zeros(0, np.int64),
               starts=np.zeros(1, np.int64))
    if not len(tid):
        return out
    flo, fhi = _floor_cell(lo[tid], inv), _floor_cell(hi[tid], inv)
    blo, bhi = _floor_cell(lo[tid].min(0), inv), _floor_cell(hi[tid].max(0), inv)
    if not (np.isfinite(blo).all() and np.isfinite(bhi).all() and (np.abs(blo) <= MAX_CELL).all() and (np.abs(bhi) <= MAX_CELL).all()):
        raise ValueError("the mesh's box leaves the grid's bound of 2^18 cells from the origin")
    min_b = blo.astype(np.int64)
    div = bhi.astype(np.int64) - min_b + 1
    ilo, ihi = (flo - min_b.astype(F)).astype(np.int64), (fhi - min_b.astype(F)).astype(np.int64)
    span = ihi - ilo + 1
    pairs = min(sum(int(s[0]) * int(s[1]) * int(s[2]) for s in span), (1 << 64) - 1)
    out.update(grid=np.concatenate([min_b, div]), pairs=pairs, min_b=min_b, div=div)
    if max_pairs is not None and pairs > max_pairs:
        raise ValueError("the mesh needs more pairs than max_pairs", pairs)
    keys, tris = [], []
    for s in np.unique(span, axis=0):                        # the triangles of one span shape together
        who = np.nonzero((span == s).all(1))[0]
        dz, dy, dx = np.meshgrid(np.arange(s[2]), np.arange(s[1]), np.arange(s[0]), indexing="ij")
        x = ilo[who, 0][:, None] + dx.ravel()[None]
        y = ilo[who, 1][:, None] + dy.ravel()[None]
        z = ilo[who, 2][:, None] + dz.ravel()[None]
        keys.append((x + y * div[0] + z * div[0] * div[1]).ravel())
        tris.append(np.repeat(tid[who], dx.size))
    keys, tris = np.concatenate(keys), np.concatenate(tris)
    order = np.lexsort((tris, keys))
    keys, tris = keys[order], tris[order]
    ukeys, starts, sizes = np.unique(keys, return_index=True, return_counts=True)
    out.update(keys=keys, tris=tris, ukeys=ukeys, starts=np.r_[starts, len(keys)].astype(np.int64), cells=len(ukeys), longest_run=int(sizes.max()))
    return out


def candidates(pl, points):
    """the total length of the runs of the 27 cells around each query's own that lie in the grid, uint32 [n]; 0 for a query with a
    non-finite coordinate or more than one cell outside the grid"""
    q = np.asarray(points, F).reshape(-1, 3)
    out = np.zeros(len(q), np.int64)
    if pl["cells"] == 0 or not len(q):
        return out.astype(U32)
    with np.errstate(invalid="ignore", over="ignore"):
        rel = _floor_cell(q, pl["inv"]) - pl["min_b"].astype(F)            # float32, as the kernel forms it
        walk = np.isfinite(q).all(1) & ((rel >= -1) & (rel <= pl["div"].astype(F))).all(1)
    who = np.nonzero(walk)[0]
    c = rel[who].astype(np.int64)
    div, sizes = pl["div"], np.diff(pl["starts"])
    for dk in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                i, j, k = c[:, 0] + di, c[:, 1] + dj, c[:, 2] + dk
                ok = (i >= 0) & (i < div[0]) & (j >= 0) & (j < div[1]) & (k >= 0) & (k < div[2])
                key = i + j * div[0] + k * div[0] * div[1]
                pos = np.minimum(np.searchsorted(pl["ukeys"], key), pl["cells"] - 1)
                hit = ok & (pl["ukeys"][pos] == key)
                out[who[hit]] += sizes[pos[hit]]
    return out.astype(U32)


def plan_loop(vertices, triangles, d_max, cell=None):
    """the grid as a dictionary (i, j, k) -> list of triangles, in absolute cell coordinates, built triangle after triangle"""
    v, t = prepare(vertices, triangles)
    inv = F(1.0) / cell_size(d_max, cell)
    cells = {}
    for ti in range(len(t)):
        c = v[t[ti]]
        if not np.isfinite(c).all():
            continue
        lo = [int(np.floor(F(c[:, a].min()) * inv)) for a in range(3)]
        hi = [int(np.floor(F(c[:, a].max()) * inv)) for a in range(3)]
        for k in range(lo[2], hi[2] + 1):
            for j in range(lo[1], hi[1] + 1):
                for i in range(lo[0], hi[0] + 1):
                    cells.setdefault((i, j, k), []).append(ti)
    return dict(inv=inv, cells=cells)


def candidates_loop(pl, points):
    q = np.asarray(points, F).reshape(-1, 3)
    out = np.zeros(len(q), U32)
    for n, p in enumerate(q):
        if not np.isfinite(p).all():
            continue
        with np.errstate(over="ignore"):
            f = np.floor(p * pl["inv"])
        if not np.isfinite(f).all():
            continue
        i0, j0, k0 = (int(x) for x in f)
        out[n] = sum(len(pl["cells"].get((i0 + di, j0 + dj, k0 + dk), ())) for dk in (-1, 0, 1) for dj in (-1, 0, 1) for di in (-1, 0, 1))
    return out
