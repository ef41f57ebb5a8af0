"""numpy restatement of the edge-split contract (include/rgbid_refine.h), steps 2 - 5, stated twice: vectorised
(np.unique over the undirected key, which is the ascending (lo, hi) order, cumulative sums for the ranks and the bases, one block of rows
per split pattern) and as plain scalar loops over dictionaries (`*_loop`).  Both are written from the contract, not from the kernels.
Only integers decide the topology; every float is one rounding of the stated expression in Python / numpy doubles."""
import math

import numpy as np

F, U32, U8 = np.float32, np.uint32, np.uint8
PLAN_COUNTS = ("edges", "eligible", "marked", "k0", "k1", "k2", "k3", "degenerate", "new_triangles")
MAX_VERTICES, MAX_TRIANGLES = 1 << 31, 1 << 29
MAX_ROUNDS = 16


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


def _length(max_edge):
    L = float(max_edge)
    if not math.isfinite(L) or L < 0:
        raise ValueError("max_edge is a finite length >= 0")
    return L


def _selection(selection, n_t):
    if selection is None:
        return np.ones(n_t, U8)
    s = np.ascontiguousarray(selection, U8).reshape(-1)
    if len(s) != n_t:
        raise ValueError("one selection byte per triangle")
    return s


def _limits(n_v, n_t, m, e):
    if n_v + m > MAX_VERTICES or n_t + e > MAX_TRIANGLES:
        raise ValueError("the refined mesh is beyond the limits")               # step 6


# ---- the vectorised statement -----------------------------------------------------------------------------------------------------------
def _q(pa, pb):
    """step 3's expression between float32 rows: doubles, one rounding per operation"""
    with np.errstate(all="ignore"):
        d = pb.astype(np.float64) - pa.astype(np.float64)
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _mid(pa, pb):
    with np.errstate(all="ignore"):
        return ((pa.astype(np.float64) + pb.astype(np.float64)) / 2.0).astype(F)


def plan(triangles, vertices, max_edge, selection=None):
    """steps 2 and 3 -> dict(n_v, triangles int64 [n_t, 3], counts, edges int64 [n_e, 2], corner_edge int64 [n_t, 3] (-1: no edge),
    eligible bool [n_e], rank int64 [n_e] (-1: not marked), k int64 [n_t], base int64 [n_t])"""
    pos = _positions(vertices)
    n_v = len(pos)
    tri = _triangles(triangles, n_v)
    L = _length(max_edge)
    sel = _selection(selection, len(tri))
    ok = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 2] != tri[:, 0])
    a, b = tri[ok].reshape(-1), tri[ok][:, (1, 2, 0)].reshape(-1)
    key = np.minimum(a, b) * max(n_v, 1) + np.maximum(a, b)
    uniq, inverse = np.unique(key, return_inverse=True)                         # ascending key = ascending (lo, hi)
    edges = np.stack([uniq // max(n_v, 1), uniq % max(n_v, 1)], 1).reshape(-1, 2)
    corner_edge = np.full((len(tri), 3), -1, np.int64)
    corner_edge[ok] = inverse.reshape(-1, 3)
    eligible = np.zeros(len(edges), bool)
    eligible[inverse[np.repeat(sel[ok] != 0, 3)]] = True
    pa, pb = pos[edges[:, 0]], pos[edges[:, 1]]
    finite = np.isfinite(pa).all(1) & np.isfinite(pb).all(1)
    with np.errstate(all="ignore"):
        marked = eligible & finite & (_q(pa, pb) > L * L)
    rank = np.where(marked, np.cumsum(marked) - 1, -1)
    k = np.where(ok, (rank[corner_edge] >= 0).sum(1), 0) if len(edges) else np.zeros(len(tri), np.int64)
    base = np.cumsum(k) - k
    counts = [len(edges), eligible.sum(), marked.sum()] + [int((k == j).sum()) for j in range(4)] + [(~ok).sum(), k.sum()]
    _limits(n_v, len(tri), int(marked.sum()), int(k.sum()))
    return dict(n_v=n_v, triangles=tri, counts=dict(zip(PLAN_COUNTS, (int(x) for x in counts))), edges=edges, corner_edge=corner_edge,
                eligible=eligible, rank=rank.astype(np.int64), k=k.astype(np.int64), base=base.astype(np.int64))


def _unit(s):
    with np.errstate(all="ignore"):
        q = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
        good = (q != 0.0) & np.isfinite(q)
        n = np.zeros((len(s), 3), F)
        n[good] = (s[good] / np.sqrt(q[good])[:, None]).astype(F)
    return n


def emit(table, vertices, colours=None, normals=None, selection=None):
    """steps 4 and 5 -> (vertices, colours, normals, triangles uint32, selection uint8 or None)"""
    n_v, tri = table["n_v"], table["triangles"]
    n_t = len(tri)
    pos = _positions(vertices, n_v)
    me = table["edges"][table["rank"] >= 0]                                     # the marked edges in rank order
    lo, hi = me[:, 0], me[:, 1]
    out_v = np.concatenate([pos, _mid(pos[lo], pos[hi])])
    out_c = out_n = out_s = None
    if colours is not None:
        c = np.ascontiguousarray(colours, U8).reshape(-1, 3)
        out_c = np.concatenate([c, ((c[lo].astype(np.int64) + c[hi].astype(np.int64) + 1) >> 1).astype(U8)])
    if normals is not None:
        n = np.ascontiguousarray(normals, F).reshape(-1, 3)
        with np.errstate(all="ignore"):
            out_n = np.concatenate([n, _unit(n[lo].astype(np.float64) + n[hi].astype(np.float64))])
    k, base = table["k"], table["base"]
    out_t = np.zeros((n_t + int(k.sum()), 3), np.int64)
    ce = np.where(table["corner_edge"] >= 0, table["corner_edge"], 0)
    r = np.where(table["corner_edge"] >= 0, table["rank"][ce], -1) if len(table["edges"]) else np.full((n_t, 3), -1, np.int64)
    m = n_v + r                                                                 # the new vertex of every corner's edge where r >= 0
    is0 = k == 0
    out_t[:n_t][is0] = tri[is0]
    # k = 1: rotate so that the marked edge is ab
    t1 = np.flatnonzero(k == 1)
    j = (r[t1] >= 0).argmax(1)
    a, b, c_ = (tri[t1, (j + s) % 3] for s in range(3))
    mm = m[t1, j]
    out_t[t1] = np.stack([a, mm, c_], 1)
    out_t[n_t + base[t1]] = np.stack([mm, b, c_], 1)
    # k = 3
    t3 = np.flatnonzero(k == 3)
    a, b, c_ = tri[t3, 0], tri[t3, 1], tri[t3, 2]
    m0, m1, m2 = m[t3, 0], m[t3, 1], m[t3, 2]
    out_t[t3] = np.stack([a, m0, m2], 1)
    out_t[n_t + base[t3]] = np.stack([m0, b, m1], 1)
    out_t[n_t + base[t3] + 1] = np.stack([m2, m1, c_], 1)
    out_t[n_t + base[t3] + 2] = np.stack([m0, m1, m2], 1)
    # k = 2: rotate so that the unmarked edge is ca, that is, the corner after the unmarked edge's comes first
    t2 = np.flatnonzero(k == 2)
    j = ((r[t2] < 0).argmax(1) + 1) % 3
    a, b, c_ = (tri[t2, (j + s) % 3] for s in range(3))
    m0, m1 = m[t2, j], m[t2, (j + 1) % 3]
    cut_m0c = _q(out_v[m0], out_v[c_]) < _q(out_v[a], out_v[m1])                # false at a tie and with a NaN: along a - m1
    out_t[t2] = np.stack([m0, b, m1], 1)
    out_t[n_t + base[t2]] = np.where(cut_m0c[:, None], np.stack([a, m0, c_], 1), np.stack([a, m0, m1], 1))
    out_t[n_t + base[t2] + 1] = np.where(cut_m0c[:, None], np.stack([m0, m1, c_], 1), np.stack([a, m1, c_], 1))
    if selection is not None:
        s = _selection(selection, n_t)
        out_s = np.concatenate([s, np.repeat(s, k)])
    return out_v, out_c, out_n, out_t.astype(U32), out_s


# ---- the scalar statement ---------------------------------------------------------------------------------------------------------------
def _f(x):
    return float(x)


def _q1(pa, pb):
    d = [_f(pb[i]) - _f(pa[i]) for i in range(3)]                               # Python floats are IEEE doubles; a product gives inf, no error
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def _mid1(pa, pb):
    return [F((_f(pa[i]) + _f(pb[i])) / 2.0) for i in range(3)]


def plan_loop(triangles, vertices, max_edge, selection=None):
    pos = _positions(vertices)
    n_v = len(pos)
    tri = _triangles(triangles, n_v)
    L = _length(max_edge)
    sel = _selection(selection, len(tri))
    named = {}                                                                  # (lo, hi) -> is a naming triangle selected
    degenerate = 0
    for t, (a, b, c) in enumerate(tri.tolist()):
        if a == b or b == c or c == a:
            degenerate += 1
            continue
        for x, y in ((a, b), (b, c), (c, a)):
            e = (min(x, y), max(x, y))
            named[e] = named.get(e, False) or sel[t] != 0
    order = sorted(named)
    index = {e: i for i, e in enumerate(order)}
    rank, m = [], 0
    for lo, hi in order:
        pa, pb = pos[lo], pos[hi]
        is_marked = bool(named[(lo, hi)] and all(math.isfinite(_f(x)) for x in list(pa) + list(pb)) and _q1(pa, pb) > L * L)
        rank.append(m if is_marked else -1)
        m += is_marked
    corner_edge, ks, bases, e_total = [], [], [], 0
    for a, b, c in tri.tolist():
        if a == b or b == c or c == a:
            row = [-1, -1, -1]
        else:
            row = [index[(min(x, y), max(x, y))] for x, y in ((a, b), (b, c), (c, a))]
        kt = sum(1 for e in row if e >= 0 and rank[e] >= 0)
        corner_edge.append(row)
        ks.append(kt)
        bases.append(e_total)
        e_total += kt
    counts = [len(order), sum(1 for e in order if named[e]), m] + [ks.count(j) for j in range(4)] + [degenerate, e_total]
    _limits(n_v, len(tri), m, e_total)
    arr = lambda x, shape: np.array(x, np.int64).reshape(shape)
    return dict(n_v=n_v, triangles=tri, counts=dict(zip(PLAN_COUNTS, (int(x) for x in counts))), edges=arr(order, (-1, 2)),
                corner_edge=arr(corner_edge, (-1, 3)), eligible=np.array([named[e] for e in order], bool).reshape(-1), rank=arr(rank, (-1,)),
                k=arr(ks, (-1,)), base=arr(bases, (-1,)))


def emit_loop(table, vertices, colours=None, normals=None, selection=None):
    n_v, tri = table["n_v"], table["triangles"]
    n_t = len(tri)
    pos = _positions(vertices, n_v)
    rank, edges = table["rank"].tolist(), table["edges"].tolist()
    new_v, new_c, new_n = [], [], []
    for e, (lo, hi) in enumerate(edges):
        if rank[e] < 0:
            continue
        new_v.append(_mid1(pos[lo], pos[hi]))
        if colours is not None:
            new_c.append([(int(colours[lo][i]) + int(colours[hi][i]) + 1) >> 1 for i in range(3)])
        if normals is not None:
            with np.errstate(all="ignore"):
                s = [np.float64(normals[lo][i]) + np.float64(normals[hi][i]) for i in range(3)]
                q = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
                new_n.append([F(x / np.sqrt(q)) for x in s] if q != 0.0 and np.isfinite(q) else [F(0), F(0), F(0)])
    cat = lambda old, new, dtype: np.concatenate([np.ascontiguousarray(old, dtype).reshape(-1, 3), np.array(new, dtype).reshape(-1, 3)])
    out_v = cat(pos, new_v, F)
    first, more, more_s = [], [], []
    for t, (a, b, c) in enumerate(tri.tolist()):
        row = table["corner_edge"][t].tolist()
        r = [rank[e] if e >= 0 else -1 for e in row]
        m = [n_v + x for x in r]
        kt = sum(1 for x in r if x >= 0)
        if kt == 0:
            rows = [(a, b, c)]
        elif kt == 1:
            if r[1] >= 0:
                a, b, c, m = b, c, a, m[1:] + m[:1]
            elif r[2] >= 0:
                a, b, c, m = c, a, b, m[2:] + m[:2]
            rows = [(a, m[0], c), (m[0], b, c)]
        elif kt == 3:
            rows = [(a, m[0], m[2]), (m[0], b, m[1]), (m[2], m[1], c), (m[0], m[1], m[2])]
        else:
            if r[0] < 0:                                                        # ab is unmarked: it becomes ca
                a, b, c, m = b, c, a, m[1:] + m[:1]
            elif r[1] < 0:
                a, b, c, m = c, a, b, m[2:] + m[:2]
            rows = [(m[0], b, m[1])]
            if _q1(out_v[m[0]], out_v[c]) < _q1(out_v[a], out_v[m[1]]):
                rows += [(a, m[0], c), (m[0], m[1], c)]
            else:
                rows += [(a, m[0], m[1]), (a, m[1], c)]
        first.append(rows[0])
        more += rows[1:]
        if selection is not None:
            more_s += [int(selection[t])] * (len(rows) - 1)
    out_t = np.array(first + more, np.int64).reshape(-1, 3).astype(U32)
    out_s = None if selection is None else np.concatenate([_selection(selection, n_t), np.array(more_s, U8).reshape(-1)])
    return (out_v, None if colours is None else cat(colours, new_c, U8), None if normals is None else cat(normals, new_n, F), out_t, out_s)


# ---- rounds -----------------------------------------------------------------------------------------------------------------------------
def refine(vertices, colours, triangles, normals, max_edge, rounds=4, selection=None, loop=False):
    """the one-shot: at most `rounds` plan-and-emit rounds, stopping at the first plan without a marked edge, one more plan when the
    rounds ran out -> (vertices, colours, triangles, normals, selection, figures) with figures = dict(rounds = the counts of every plan
    that was emitted, rounds_run, left = the marked edges of the last plan)"""
    if isinstance(rounds, bool) or int(rounds) != rounds or not 0 <= rounds <= MAX_ROUNDS:
        raise ValueError("rounds is an integer in 0 .. 16")
    p, e = (plan_loop, emit_loop) if loop else (plan, emit)
    v = _positions(vertices)
    t = _triangles(triangles, len(v)).astype(U32)
    c = None if colours is None else np.ascontiguousarray(colours, U8).reshape(-1, 3)
    n = None if normals is None else np.ascontiguousarray(normals, F).reshape(-1, 3)
    s = _selection(selection, len(t))
    per_round, left = [], 0
    for _ in range(int(rounds)):
        table = p(t, v, max_edge, s)
        left = table["counts"]["marked"]
        if left == 0:
            break
        per_round.append(table["counts"])
        v, c, n, t, s = e(table, v, c, n, s)
    else:
        left = p(t, v, max_edge, s)["counts"]["marked"]
    return v, c, t, n, s, dict(rounds=per_round, rounds_run=len(per_round), left=left)


def same(a, b):
    """the indices at which two tuples of arrays (or None) differ in type, shape or bytes"""
    return [i for i, (x, y) in enumerate(zip(a, b)) if (x is None) != (y is None) or (x is not None and _differ(x, y))]


def _differ(x, y):
    return x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes()


def same_table(a, b):
    """the keys at which two plans differ"""
    return [k for k in a if (a[k] != b[k] if isinstance(a[k], (dict, int)) else _differ(np.asarray(a[k]), np.asarray(b[k])))]
