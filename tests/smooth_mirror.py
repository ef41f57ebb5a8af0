"""numpy restatement of the smoothing contract (include/rgbid_smooth.h), steps 1 - 6, stated twice: vectorised
(np.unique for the pairs, np.add.at for the sums, which adds one element after the other in index order; np.add.reduceat and np.sum are
pairwise over eight elements and more and would not do) and as plain scalar loops over dictionaries (`*_loop`).  Both are written from the
contract, not from the kernels.  Only integers decide the topology; the sums are Python / numpy doubles, one rounding per operation."""
import math

import numpy as np

F, U32 = np.float32, np.uint32
COUNTS = ("pairs", "edges", "boundary_pairs", "boundary_vertices", "isolated", "max_degree", "dropped", "non_manifold")
FROM, TO = (0, 1, 1, 2, 2, 0), (1, 0, 2, 1, 0, 2)             # the six ordered corner pairs of a triangle


def _triangles(triangles, n_v):
    tri = np.ascontiguousarray(np.asarray(triangles).reshape(-1, 3)).astype(np.int64)
    if len(tri) and (tri.min() < 0 or tri.max() >= n_v):
        raise ValueError("a triangle names a vertex that does not exist")      # step 1: the mesh is refused
    return tri


def _positions(vertices, n_v=None):
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    if n_v is not None and len(v) != n_v:
        raise ValueError("one position per vertex")
    return v


# ---- the vectorised statement -----------------------------------------------------------------------------------------------------------
def adjacency(triangles, n_v):
    """steps 2 and 3 -> dict(n_v, triangles int64 [n_t, 3], offsets uint32 [n_v + 1], neighbours uint32 [P], incidences uint32 [P], boundary
    uint8 [n_v], rows int64 [P] (the vertex of every row), corner_offsets uint32 [n_v + 1], corners uint32 [3 n_t], counts dict)"""
    tri = _triangles(triangles, n_v)
    v, u = tri[:, FROM].reshape(-1), tri[:, TO].reshape(-1)
    keep = v != u
    uniq, inc = np.unique(v[keep] * max(n_v, 1) + u[keep], return_counts=True)      # below 2^62: int64 holds it
    rows, nbr = uniq // max(n_v, 1), uniq % max(n_v, 1)
    offsets = np.searchsorted(rows, np.arange(n_v + 1), "left")
    boundary = np.zeros(n_v, np.uint8)
    boundary[rows[inc == 1]] = 1
    degree = np.diff(offsets)
    flat = tri.reshape(-1)
    corners = np.argsort(flat, kind="stable")
    counts = dict(pairs=len(uniq), edges=len(uniq) // 2, boundary_pairs=int((inc == 1).sum()), boundary_vertices=int(boundary.sum()),
                  isolated=int((degree == 0).sum()), max_degree=int(degree.max()) if n_v else 0, dropped=int((~keep).sum()),
                  non_manifold=int((inc >= 3).sum()))
    return dict(n_v=n_v, triangles=tri, offsets=offsets.astype(U32), neighbours=nbr.astype(U32), incidences=inc.astype(U32), boundary=boundary,
                rows=rows, corner_offsets=np.searchsorted(flat[corners], np.arange(n_v + 1), "left").astype(U32), corners=corners.astype(U32),
                counts=counts)


def smooth_pass(pos, adj, f, pin_boundary=False):
    """step 4: one pass with factor f from `pos` to a new array"""
    pos = _positions(pos, adj["n_v"])
    rows, nbr = adj["rows"], adj["neighbours"].astype(np.int64)
    fin = np.isfinite(pos).all(1)
    ok = fin[nbr]
    s = np.zeros((len(pos), 3), np.float64)
    for a in range(3):
        np.add.at(s[:, a], rows[ok], pos[nbr[ok], a].astype(np.float64))     # sequential adds, a row's neighbours in ascending u
    k = np.bincount(rows[ok], minlength=len(pos))
    move = fin & (k > 0)
    if pin_boundary:
        move &= adj["boundary"] == 0
    out = pos.copy()                                            # a vertex that does not move keeps its words
    x = pos[move].astype(np.float64)
    m = s[move] / k[move].astype(np.float64)[:, None]
    with np.errstate(over="ignore"):
        out[move] = (x + np.float64(f) * (m - x)).astype(F)
    return out


def smooth(vertices, triangles, iterations, lam=0.5, mu=-0.53, pin_boundary=False, adj=None):
    """step 5 -> positions float32 [n_v, 3]"""
    pos = _positions(vertices)
    adj = adjacency(triangles, len(pos)) if adj is None else adj
    if not (0 <= iterations <= 4096 and math.isfinite(lam) and 0 < lam <= 1 and math.isfinite(mu) and -2 <= mu <= 0):
        raise ValueError("an argument outside step 5")
    out = pos.copy()
    for _ in range(iterations):
        out = smooth_pass(out, adj, lam, pin_boundary)
        if mu != 0:
            out = smooth_pass(out, adj, mu, pin_boundary)
    return out


def normals(vertices, adj):
    """step 6 -> float32 [n_v, 3]"""
    pos = _positions(vertices, adj["n_v"])
    tri = adj["triangles"]
    s = np.zeros((len(pos), 3), np.float64)
    if len(tri):
        meas = np.isfinite(pos).all(1)[tri].all(1)
        with np.errstate(invalid="ignore"):                     # a signalling NaN, inf - inf: triangles that are not measurable
            p = pos.astype(np.float64)[tri]
            e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
            area = np.stack([(e1[:, 1] * e2[:, 2]) - (e1[:, 2] * e2[:, 1]), (e1[:, 2] * e2[:, 0]) - (e1[:, 0] * e2[:, 2]),
                             (e1[:, 0] * e2[:, 1]) - (e1[:, 1] * e2[:, 0])], 1)
        corner_ok = np.repeat(meas, 3)                          # the corners 3 t + c in ascending order: every vertex's own order
        for a in range(3):
            np.add.at(s[:, a], tri.reshape(-1)[corner_ok], np.repeat(area[:, a], 3)[corner_ok])
    with np.errstate(all="ignore"):
        q = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
        good = (q != 0) & np.isfinite(q)
        return np.where(good[:, None], s / np.sqrt(q)[:, None], 0.0).astype(F)


# ---- the second statement: scalar loops ----------------------------------------------------------------------------------------------------
def adjacency_loop(triangles, n_v):
    tri = _triangles(triangles, n_v)
    pairs, dropped = {}, 0
    at = [[] for _ in range(n_v)]
    for t, row in enumerate(tri.tolist()):
        for a, b in zip(FROM, TO):
            if row[a] == row[b]:
                dropped += 1
            else:
                pairs[(row[a], row[b])] = pairs.get((row[a], row[b]), 0) + 1
        for c in range(3):
            at[row[c]].append(3 * t + c)
    offsets, nbr, inc, rows, boundary = [0], [], [], [], [0] * n_v
    keys = sorted(pairs)
    j = 0
    for v in range(n_v):
        while j < len(keys) and keys[j][0] == v:
            nbr.append(keys[j][1])
            inc.append(pairs[keys[j]])
            rows.append(v)
            if pairs[keys[j]] == 1:
                boundary[v] = 1
            j += 1
        offsets.append(len(nbr))
    degree = [offsets[v + 1] - offsets[v] for v in range(n_v)]
    corner_offsets, corners = [0], []
    for v in range(n_v):
        corners += at[v]
        corner_offsets.append(len(corners))
    counts = dict(pairs=len(nbr), edges=len(nbr) // 2, boundary_pairs=inc.count(1), boundary_vertices=sum(boundary), isolated=degree.count(0),
                  max_degree=max(degree) if degree else 0, dropped=dropped, non_manifold=sum(1 for i in inc if i >= 3))
    return dict(n_v=n_v, triangles=tri, offsets=np.array(offsets, U32), neighbours=np.array(nbr, U32), incidences=np.array(inc, U32),
                boundary=np.array(boundary, np.uint8), rows=np.array(rows, np.int64), corner_offsets=np.array(corner_offsets, U32),
                corners=np.array(corners, U32), counts=counts)


def _finite(row):
    return all(math.isfinite(float(x)) for x in row)


def smooth_pass_loop(pos, adj, f, pin_boundary=False):
    pos = _positions(pos, adj["n_v"])
    out = pos.copy()
    off, nbr = adj["offsets"].tolist(), adj["neighbours"].tolist()
    fin = [_finite(r) for r in pos]
    for v in range(len(pos)):
        if not fin[v] or (pin_boundary and adj["boundary"][v]):
            continue
        s, k = [0.0, 0.0, 0.0], 0
        for u in nbr[off[v]:off[v + 1]]:
            if fin[u]:
                for a in range(3):
                    s[a] += float(pos[u, a])
                k += 1
        if k == 0:
            continue
        for a in range(3):
            x = float(pos[v, a])
            m = s[a] / float(k)
            with np.errstate(over="ignore"):
                out[v, a] = F(x + f * (m - x))
    return out


def smooth_loop(vertices, triangles, iterations, lam=0.5, mu=-0.53, pin_boundary=False, adj=None):
    pos = _positions(vertices)
    adj = adjacency_loop(triangles, len(pos)) if adj is None else adj
    out = pos.copy()
    for _ in range(iterations):
        out = smooth_pass_loop(out, adj, float(lam), pin_boundary)
        if mu != 0:
            out = smooth_pass_loop(out, adj, float(mu), pin_boundary)
    return out


def normals_loop(vertices, adj):
    pos = _positions(vertices, adj["n_v"])
    tri = adj["triangles"].tolist()
    off, corners = adj["corner_offsets"].tolist(), adj["corners"].tolist()
    fin = [_finite(r) for r in pos]
    out = np.zeros((len(pos), 3), F)
    for v in range(len(pos)):
        s = [0.0, 0.0, 0.0]
        for c in corners[off[v]:off[v + 1]]:
            i = tri[c // 3]
            if not (fin[i[0]] and fin[i[1]] and fin[i[2]]):
                continue
            p = [[float(pos[i[k], a]) for a in range(3)] for k in range(3)]
            e1 = [p[1][a] - p[0][a] for a in range(3)]
            e2 = [p[2][a] - p[0][a] for a in range(3)]
            s[0] += (e1[1] * e2[2]) - (e1[2] * e2[1])
            s[1] += (e1[2] * e2[0]) - (e1[0] * e2[2])
            s[2] += (e1[0] * e2[1]) - (e1[1] * e2[0])
        q = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
        if q != 0.0 and math.isfinite(q):
            out[v] = [F(s[a] / math.sqrt(q)) for a in range(3)]
    return out


def same_adjacency(a, b):
    """the names of the entries in which two adjacencies differ in a byte"""
    bad = [k for k in ("offsets", "neighbours", "incidences", "boundary", "corner_offsets", "corners")
           if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    return bad + (["counts"] if a["counts"] != b["counts"] else [])
