"""numpy restatement of the hole-filling contract (include/rgbid_holes.h), steps 2 - 5, stated twice: vectorised
(np.unique over the undirected key, successor arrays, pointer doubling for the labels, a walk from the heads for the order, np.add.at for
the sums, which adds one element after the other in index order; np.add.reduceat and np.sum are pairwise and would not do) and as plain
scalar loops over dictionaries (`*_loop`).  Both are written from the contract, not from the kernels.  Only integers decide the topology;
the sums are Python / numpy doubles, one rounding per operation."""
import math

import numpy as np

F, U32, U8 = np.float32, np.uint32, np.uint8
PLAN_COUNTS = ("directed_edges", "boundary_half_edges", "boundary_vertices", "non_simple", "loops", "loop_edges", "blocked", "longest")
SELECT_COUNTS = ("too_long", "not_finite", "outlines", "filled", "new_triangles")
FILLED, TOO_LONG, NOT_FINITE, OUTLINE = 0, 1, 2, 3
MAX_VERTICES, MAX_TRIANGLES = 1 << 31, 1 << 29


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


def _table(n_v, tri, counts, offsets, vertices, owners):
    return dict(n_v=n_v, triangles=tri, counts=dict(zip(PLAN_COUNTS, (int(x) for x in counts))), offsets=np.array(offsets, U32).reshape(-1),
                vertices=np.array(vertices, U32).reshape(-1), owners=np.array(owners, U32).reshape(-1))


# ---- the vectorised statement -----------------------------------------------------------------------------------------------------------
def plan(triangles, n_v):
    """steps 2 and 3 -> dict(n_v, triangles int64 [n_t, 3], counts, offsets uint32 [L + 1], vertices uint32 [S], owners uint32 [S])"""
    tri = _triangles(triangles, n_v)
    ok = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 2] != tri[:, 0])
    corner = np.arange(3 * len(tri), dtype=np.int64).reshape(-1, 3)[ok].reshape(-1)
    a, b = tri[ok].reshape(-1), tri[ok][:, (1, 2, 0)].reshape(-1)
    _, first, cnt = np.unique(np.minimum(a, b) * max(n_v, 1) + np.maximum(a, b), return_index=True, return_counts=True)
    lone = first[cnt == 1]                                      # named by exactly one corner, in either direction
    ba, bb, bo = a[lone], b[lone], corner[lone]
    out, inn = np.bincount(ba, minlength=n_v), np.bincount(bb, minlength=n_v)
    simple = (out == 1) & (inn == 1)
    succ, owner = np.full(n_v, -1, np.int64), np.full(n_v, -1, np.int64)
    leaves = simple[ba]
    succ[ba[leaves]], owner[ba[leaves]] = bb[leaves], bo[leaves]
    sv = np.flatnonzero(simple)
    # the minimum label over the next 2^j successors, the OR of "runs into a vertex that is not simple", the jump
    label, jump = sv.copy(), succ[sv]
    blocked = ~simple[jump]
    jump = np.where(blocked, sv, jump)
    item = np.full(n_v, -1, np.int64)
    item[sv] = np.arange(len(sv))
    for _ in range(int(len(sv)).bit_length()):
        j = item[jump]
        label, blocked, jump = np.minimum(label, label[j]), blocked | blocked[j], jump[j]
    heads = sv[~blocked & (label == sv)]                        # ascending v_0
    cols_l, cols_v = [], []
    loop, cur = np.arange(len(heads)), heads.copy()
    while len(loop):                                            # a walk from every head at once, one hop per trip
        cols_l.append(loop)
        cols_v.append(cur)
        cur = succ[cur]
        go = cur != heads[loop]
        loop, cur = loop[go], cur[go]
    ls = np.concatenate(cols_l) if cols_l else np.zeros(0, np.int64)
    vs = np.concatenate(cols_v) if cols_v else np.zeros(0, np.int64)
    order = np.argsort(ls, kind="stable")                       # the hops of a loop stay in their order
    k = np.bincount(ls, minlength=len(heads))
    s = int(k.sum())
    bverts = (out + inn) > 0
    counts = (len(a), len(lone), bverts.sum(), (bverts & ~simple).sum(), len(heads), s, len(lone) - s, k.max() if len(k) else 0)
    return _table(n_v, tri, counts, np.concatenate([[0], np.cumsum(k)]), vs[order], owner[vs[order]])


def _cross(u, w):
    return np.stack([(u[:, 1] * w[:, 2]) - (u[:, 2] * w[:, 1]), (u[:, 2] * w[:, 0]) - (u[:, 0] * w[:, 2]), (u[:, 0] * w[:, 1]) - (u[:, 1] * w[:, 0])], 1)


def _ordered_sums(rows, values, n):
    s = np.zeros((n, values.shape[1]), np.float64)
    for a in range(values.shape[1]):
        np.add.at(s[:, a], rows, values[:, a])                  # sequential adds, a loop's vertices in loop order
    return s


def select(table, vertices, max_edges=64, any_facing=False):
    """step 4 -> dict(status uint8 [L], centres float32 [L, 3] (those of the filled loops count), counts)"""
    if not 3 <= max_edges <= (1 << 31) - 1:
        raise ValueError("max_edges outside step 4")
    pos = _positions(vertices, table["n_v"])
    off, lv, tri = table["offsets"].astype(np.int64), table["vertices"].astype(np.int64), table["triangles"]
    n_l = len(off) - 1
    k = np.diff(off)
    rows = np.repeat(np.arange(n_l), k)
    nxt = np.arange(len(lv)) + 1
    nxt[off[1:] - 1] = off[:-1]                                 # i + 1 mod k
    with np.errstate(all="ignore"):
        p = pos.astype(np.float64)
        s = _ordered_sums(rows, p[lv], n_l)
        m = (s / k.astype(np.float64)[:, None]).astype(F)
        c = m.astype(np.float64)
        finite = np.ones(n_l, bool)
        np.logical_and.at(finite, rows, np.isfinite(pos).all(1)[lv])
        A = _ordered_sums(rows, _cross(p[lv] - p[lv[nxt]], c[rows] - p[lv[nxt]]), n_l)
        q = p[tri[table["owners"].astype(np.int64) // 3]] if len(lv) else np.zeros((0, 3, 3))
        N = _ordered_sums(rows, _cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]), n_l)
        faces = ((A[:, 0] * N[:, 0] + A[:, 1] * N[:, 1]) + A[:, 2] * N[:, 2]) > 0
    status = np.full(n_l, FILLED, U8)
    if not any_facing:
        status[~faces] = OUTLINE
    status[~finite] = NOT_FINITE
    status[k > max_edges] = TOO_LONG
    return _selection(table, status, m, k)


def _selection(table, status, centres, k):
    filled = status == FILLED
    counts = dict(too_long=int((status == TOO_LONG).sum()), not_finite=int((status == NOT_FINITE).sum()), outlines=int((status == OUTLINE).sum()),
                  filled=int(filled.sum()), new_triangles=int(np.asarray(k)[filled].sum()))
    if table["n_v"] + counts["filled"] > MAX_VERTICES or len(table["triangles"]) + counts["new_triangles"] > MAX_TRIANGLES:
        raise ValueError("the filled mesh is beyond step 1")
    return dict(status=status, centres=np.array(centres, F).reshape(-1, 3), counts=counts)


def _unit(s):
    with np.errstate(all="ignore"):
        q = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
        good = (q != 0) & np.isfinite(q)
        return np.where(good[:, None], s / np.sqrt(q)[:, None], 0.0).astype(F)


def emit(table, sel, vertices, colours=None, normals=None):
    """step 5 -> (vertices float32 [n_v + F, 3], colours uint8 or None, normals float32 or None, triangles uint32 [n_t + E, 3])"""
    pos = _positions(vertices, table["n_v"])
    n_v, tri = table["n_v"], table["triangles"]
    off, lv = table["offsets"].astype(np.int64), table["vertices"].astype(np.int64)
    fl = np.flatnonzero(sel["status"] == FILLED)
    k = np.diff(off)[fl]
    rows = np.repeat(np.arange(len(fl)), k)                     # the rank of every new triangle's loop
    base = np.concatenate([[0], np.cumsum(k)])[:-1]
    i = np.arange(len(rows)) - base[rows]
    at = off[fl][rows] + i
    at_next = off[fl][rows] + (i + 1) % k[rows]
    fans = np.stack([lv[at_next], lv[at], n_v + rows], 1) if len(rows) else np.zeros((0, 3), np.int64)
    out_v = np.concatenate([pos, sel["centres"][fl]]).astype(F)
    out_t = np.concatenate([tri, fans]).astype(U32)
    out_c = out_n = None
    if colours is not None:
        col = np.ascontiguousarray(colours, U8).reshape(n_v, 3)
        sums = np.zeros((len(fl), 3), np.int64)
        np.add.at(sums, rows, col[lv[at]].astype(np.int64))
        out_c = np.concatenate([col, ((2 * sums + k[:, None]) // (2 * k[:, None])).astype(U8)])
    if normals is not None:
        nrm = _positions(normals, n_v)
        out_n = np.concatenate([nrm, _unit(_ordered_sums(rows, nrm[lv[at]].astype(np.float64), len(fl)))])
    return out_v, out_c, out_n, out_t


def fill(vertices, colours, triangles, normals, max_edges=64, any_facing=False, loop=False):
    """the one-shot, as rgbid.holes.fill_holes -> (vertices, colours, triangles, normals, figures)"""
    pos = _positions(vertices)
    table = (plan_loop if loop else plan)(triangles, len(pos))
    sel = (select_loop if loop else select)(table, pos, max_edges, any_facing)
    v, c, n, t = (emit_loop if loop else emit)(table, sel, pos, colours, normals)
    return v, c, t, n, dict(table["counts"], **sel["counts"])


# ---- the second statement: scalar loops ----------------------------------------------------------------------------------------------------
def plan_loop(triangles, n_v):
    tri = _triangles(triangles, n_v)
    n = {}
    rows = tri.tolist()
    for r in rows:
        if r[0] != r[1] and r[1] != r[2] and r[2] != r[0]:
            for c in range(3):
                e = (r[c], r[(c + 1) % 3])
                n[e] = n.get(e, 0) + 1
    out, inn, succ, owner = {}, {}, {}, {}
    n_b = 0
    for t, r in enumerate(rows):
        if r[0] != r[1] and r[1] != r[2] and r[2] != r[0]:
            for c in range(3):
                a, b = r[c], r[(c + 1) % 3]
                if n[(a, b)] + n.get((b, a), 0) == 1:
                    n_b += 1
                    out[a] = out.get(a, 0) + 1
                    inn[b] = inn.get(b, 0) + 1
                    succ[a], owner[a] = b, 3 * t + c            # read for a simple a only: then it has one
    bverts = sorted(set(out) | set(inn))
    simple = {v for v in bverts if out.get(v, 0) == 1 and inn.get(v, 0) == 1}
    seen = set()
    offsets, vertices, owners, longest = [0], [], [], 0
    for v0 in sorted(simple):                                   # the first unseen vertex of a loop is its smallest
        if v0 in seen:
            continue
        chain, v = [], v0
        while v in simple and v not in seen:
            seen.add(v)
            chain.append(v)
            v = succ[v]
        if v == v0:
            vertices += chain
            owners += [owner[u] for u in chain]
            offsets.append(len(vertices))
            longest = max(longest, len(chain))
    counts = (sum(n.values()), n_b, len(bverts), len(bverts) - len(simple), len(offsets) - 1, len(vertices), n_b - len(vertices), longest)
    return _table(n_v, tri, counts, offsets, vertices, owners)


def _cross3(u, w):
    return [(u[1] * w[2]) - (u[2] * w[1]), (u[2] * w[0]) - (u[0] * w[2]), (u[0] * w[1]) - (u[1] * w[0])]


def select_loop(table, vertices, max_edges=64, any_facing=False):
    pos = _positions(vertices, table["n_v"])
    p = pos.astype(np.float64).tolist()
    off, lv, lo, tri = table["offsets"].tolist(), table["vertices"].tolist(), table["owners"].tolist(), table["triangles"].tolist()
    status, centres, ks = [], [], []
    with np.errstate(all="ignore"):
        for l in range(len(off) - 1):
            vs = lv[off[l]:off[l + 1]]
            k = len(vs)
            ks.append(k)
            if k > max_edges:
                status.append(TOO_LONG)
                centres.append([F(0)] * 3)
                continue
            s = [0.0, 0.0, 0.0]
            for v in vs:
                for a in range(3):
                    s[a] += p[v][a]
            m = [F(np.float64(s[a]) / np.float64(k)) for a in range(3)]
            centres.append(m)
            c = [float(x) for x in m]
            A, N = [0.0] * 3, [0.0] * 3
            for i, v in enumerate(vs):
                w = vs[(i + 1) % k]
                x = _cross3([p[v][a] - p[w][a] for a in range(3)], [c[a] - p[w][a] for a in range(3)])
                q = [p[j] for j in tri[lo[off[l] + i] // 3]]
                y = _cross3([q[1][a] - q[0][a] for a in range(3)], [q[2][a] - q[0][a] for a in range(3)])
                for a in range(3):
                    A[a] += x[a]
                    N[a] += y[a]
            if not all(math.isfinite(x) for v in vs for x in p[v]):
                status.append(NOT_FINITE)
            elif not any_facing and not (A[0] * N[0] + A[1] * N[1]) + A[2] * N[2] > 0:
                status.append(OUTLINE)
            else:
                status.append(FILLED)
    return _selection(table, np.array(status, U8).reshape(-1), centres, np.array(ks, np.int64).reshape(-1))


def emit_loop(table, sel, vertices, colours=None, normals=None):
    pos = _positions(vertices, table["n_v"])
    n_v = table["n_v"]
    off, lv = table["offsets"].tolist(), table["vertices"].tolist()
    new_v, new_t, new_c, new_n = [], [], [], []
    for l, st in enumerate(sel["status"].tolist()):
        if st != FILLED:
            continue
        vs = lv[off[l]:off[l + 1]]
        k, r = len(vs), len(new_v)
        new_v.append(sel["centres"][l])
        new_t += [(vs[(i + 1) % k], vs[i], n_v + r) for i in range(k)]
        if colours is not None:
            new_c.append([(2 * sum(int(colours[v][a]) for v in vs) + k) // (2 * k) for a in range(3)])
        if normals is not None:
            s = [0.0, 0.0, 0.0]
            for v in vs:
                for a in range(3):
                    s[a] += float(normals[v][a])
            with np.errstate(all="ignore"):
                q = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
                new_n.append([F(s[a] / math.sqrt(q)) for a in range(3)] if q != 0.0 and math.isfinite(q) else [F(0)] * 3)
    cat = lambda old, new, dtype: np.concatenate([np.asarray(old, dtype).reshape(-1, 3), np.array(new, dtype).reshape(-1, 3)])
    return (cat(pos, new_v, F), None if colours is None else cat(colours, new_c, U8), None if normals is None else cat(normals, new_n, F),
            cat(table["triangles"], new_t, U32))


def same(a, b):
    """the names of the entries in which two tables, selections or emitted meshes differ in a byte"""
    if isinstance(a, dict):
        keys = [k for k in a if isinstance(a[k], np.ndarray) and k != "triangles"]
        bad = [k for k in keys if k != "centres" and _differ(a[k], b[k])]
        if "centres" in a:
            f = a["status"] == FILLED
            bad += ["centres"] if _differ(a["centres"][f], b["centres"][f]) else []
        return bad + (["counts"] if a["counts"] != b["counts"] else [])
    return [i for i, (x, y) in enumerate(zip(a, b)) if (x is None) != (y is None) or (x is not None and _differ(x, y))]


def _differ(x, y):
    return x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes()
