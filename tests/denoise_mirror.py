"""numpy restatement of the denoising contract (include/rgbid_denoise.h), steps 2 - 7, stated twice: vectorised
(a stable argsort for the face table, np.unique for the neighbourhoods, np.add.at for the sums, which adds one element after the other in
index order; np.add.reduceat and np.sum are pairwise over eight elements and more and would not do) and as plain scalar loops over
dictionaries (`*_loop`).  Both are written from the contract, not from the kernels.  Only integers decide the topology; the sums are
Python / numpy doubles, one rounding per operation."""
import math

import numpy as np

F, U32 = np.float32, np.uint32
COUNTS = ("empty_rows", "longest_row", "repeating_triangles", "work")
MAX_ITERATIONS = 256


def _triangles(triangles, n_v):
    tri = np.ascontiguousarray(np.asarray(triangles).reshape(-1, 3)).astype(np.int64)
    if len(tri) and (tri.min() < 0 or tri.max() >= n_v):
        raise ValueError("a triangle names a vertex that does not exist")      # step 1: the mesh is refused
    return tri


def _rows3(a, rows=None, what="one position per vertex"):
    a = np.ascontiguousarray(a, F).reshape(-1, 3)
    if rows is not None and len(a) != rows:
        raise ValueError(what)
    return a


def _runs_arg(iterations, threshold=0.0):
    if not (0 <= iterations <= MAX_ITERATIONS and math.isfinite(threshold) and 0.0 <= threshold < 1.0):
        raise ValueError("an argument outside step 7")


# ---- the vectorised statement -----------------------------------------------------------------------------------------------------------
def face_table(triangles, n_v):
    """step 2 -> dict(n_v, triangles int64 [n_t, 3], offsets uint32 [n_v + 1], faces uint32 [3 n_t], counts dict)"""
    tri = _triangles(triangles, n_v)
    flat = tri.reshape(-1)
    corners = np.argsort(flat, kind="stable")                   # ascending corner number inside every vertex's row
    offsets = np.searchsorted(flat[corners], np.arange(n_v + 1), "left")
    length = np.diff(offsets)
    repeats = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 2] == tri[:, 0])
    counts = dict(empty_rows=int((length == 0).sum()), longest_row=int(length.max()) if n_v else 0, repeating_triangles=int(repeats.sum()),
                  work=int(length[flat].sum()))
    return dict(n_v=n_v, triangles=tri, offsets=offsets.astype(U32), faces=(corners // 3).astype(U32), counts=counts)


def _entries(tab):
    """the face table as (vertex, face) per entry, in the table's order"""
    off = tab["offsets"].astype(np.int64)
    return np.repeat(np.arange(tab["n_v"]), np.diff(off)), tab["faces"].astype(np.int64)


def neighbourhoods(tab):
    """step 3 -> (t, j): every member j of every F(t), ascending in t and, inside one t, in j; kept in the table"""
    if "pairs" not in tab:
        tri, off, faces = tab["triangles"], tab["offsets"].astype(np.int64), tab["faces"].astype(np.int64)
        n_t = len(tri)
        flat = tri.reshape(-1)
        length = (off[1:] - off[:-1])[flat] if n_t else np.zeros(0, np.int64)
        t = np.repeat(np.arange(3 * n_t) // 3, length)
        first = np.cumsum(length) - length
        j = faces[np.repeat(off[flat] if n_t else first, length) + (np.arange(int(length.sum())) - np.repeat(first, length))]
        both = np.unique(t * max(n_t, 1) + j)                   # below 2^58: int64 holds it
        tab["pairs"] = (both // max(n_t, 1), both % max(n_t, 1))
    return tab["pairs"]


def _unit(s, keep):
    """(float)(s / sqrt(q)) where q = (s0 s0 + s1 s1) + s2 s2 is finite and > 0, the rows of `keep` elsewhere"""
    with np.errstate(all="ignore"):
        q = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
        good = np.isfinite(q) & (q > 0)
        out = keep.copy()
        out[good] = (s[good] / np.sqrt(q[good])[:, None]).astype(F)
    return out


def raw_normals(vertices, tab):
    """step 4 -> float32 [n_t, 3]"""
    pos = _rows3(vertices, tab["n_v"])
    tri = tab["triangles"]
    s = np.zeros((len(tri), 3), np.float64)
    if len(tri):
        meas = np.isfinite(pos).all(1)[tri].all(1)
        with np.errstate(invalid="ignore"):                     # a signalling NaN, inf - inf: triangles that are not measurable
            p = pos.astype(np.float64)[tri]
            e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
            area = np.stack([(e1[:, 1] * e2[:, 2]) - (e1[:, 2] * e2[:, 1]), (e1[:, 2] * e2[:, 0]) - (e1[:, 0] * e2[:, 2]),
                             (e1[:, 0] * e2[:, 1]) - (e1[:, 1] * e2[:, 0])], 1)
        s[meas] = area[meas]
    return _unit(s, np.zeros((len(tri), 3), F))


def normal_pass(normals, tab, threshold):
    """step 5: one pass with threshold T from `normals` to a new array"""
    n = _rows3(normals, len(tab["triangles"]), "one normal per triangle")
    t, j = neighbourhoods(tab)
    T = np.float64(threshold)
    fin = np.isfinite(n).all(1)
    active = fin & (n != 0).any(1)
    s = np.zeros((len(n), 3), np.float64)
    with np.errstate(all="ignore"):
        nd = n.astype(np.float64)
        nt, nj = nd[t], nd[j]
        d = (nt[:, 0] * nj[:, 0] + nt[:, 1] * nj[:, 1]) + nt[:, 2] * nj[:, 2]
        use = active[t] & fin[j] & np.isfinite(d) & (d > T)
        w = (d - T) * (d - T)
        for k in range(3):
            np.add.at(s[:, k], t[use], (w * nj[:, k])[use])      # sequential adds, the members of one F(t) in ascending j
    return _unit(s, n)                                          # a triangle that is not active has s = 0 and keeps its words


def vertex_pass(vertices, normals, tab):
    """step 6: one pass from `vertices` to a new array with the face normals `normals`"""
    pos = _rows3(vertices, tab["n_v"])
    tri = tab["triangles"]
    N = _rows3(normals, len(tri), "one normal per triangle")
    v, f = _entries(tab)
    first = np.ones(len(f), bool)
    first[1:] = (v[1:] != v[:-1]) | (f[1:] != f[:-1])           # a repeat stands next to its first entry and counts once
    fin = np.isfinite(pos).all(1)
    part = np.isfinite(N).all(1) & (N != 0).any(1) & (fin[tri].all(1) if len(tri) else np.zeros(0, bool))
    use = first & part[f]
    v, f = v[use], f[use]
    s = np.zeros((len(pos), 3), np.float64)
    out = pos.copy()                                            # a vertex that does not move keeps its words
    with np.errstate(all="ignore"):
        p = pos.astype(np.float64)
        c = ((p[tri[f, 0]] + p[tri[f, 1]]) + p[tri[f, 2]]) / 3.0
        e = c - p[v]
        Nd = N.astype(np.float64)[f]
        dd = (Nd[:, 0] * e[:, 0] + Nd[:, 1] * e[:, 1]) + Nd[:, 2] * e[:, 2]
        for k in range(3):
            np.add.at(s[:, k], v, Nd[:, k] * dd)                 # sequential adds, a row's triangles in ascending t
        m = np.bincount(v, minlength=len(pos))
        move = fin & (m > 0)
        out[move] = (p[move] + s[move] / m[move].astype(np.float64)[:, None]).astype(F)
    return out


def normals(vertices, tab, iterations, threshold):
    """step 7: the raw normals after `iterations` normal passes -> float32 [n_t, 3]"""
    _runs_arg(iterations, threshold)
    n = raw_normals(vertices, tab)
    for _ in range(iterations):
        n = normal_pass(n, tab, threshold)
    return n


def vertices(vertices, face_normals, tab, iterations):
    """step 7: the positions after `iterations` vertex passes with the given normals -> float32 [n_v, 3]"""
    _runs_arg(iterations)
    out = _rows3(vertices, tab["n_v"]).copy()
    for _ in range(iterations):
        out = vertex_pass(out, face_normals, tab)
    return out


def denoise(verts, triangles, normal_iterations=5, vertex_iterations=10, threshold=0.4, tab=None):
    """both stages -> (positions float32 [n_v, 3], filtered face normals float32 [n_t, 3])"""
    pos = _rows3(verts)
    tab = face_table(triangles, len(pos)) if tab is None else tab
    n = normals(pos, tab, normal_iterations, threshold)
    return vertices(pos, n, tab, vertex_iterations), n


# ---- the second statement: scalar loops ----------------------------------------------------------------------------------------------------
def face_table_loop(triangles, n_v):
    tri = _triangles(triangles, n_v)
    rows = {v: [] for v in range(n_v)}
    repeats = 0
    for t, (a, b, c) in enumerate(tri.tolist()):
        for i in (a, b, c):                                     # corner 3 t + c in ascending order
            rows[i].append(t)
        repeats += len({a, b, c}) < 3
    offsets, faces = [0], []
    for v in range(n_v):
        faces += rows[v]
        offsets.append(len(faces))
    lengths = [len(rows[v]) for v in range(n_v)]
    work = sum(len(rows[i]) for row in tri.tolist() for i in row)
    counts = dict(empty_rows=lengths.count(0), longest_row=max(lengths) if lengths else 0, repeating_triangles=repeats, work=work)
    return dict(n_v=n_v, triangles=tri, offsets=np.array(offsets, U32), faces=np.array(faces, U32), counts=counts, rows=rows)


def _finite(row):
    return all(math.isfinite(float(x)) for x in row)


def _round(x):
    with np.errstate(over="ignore"):
        return F(x)


def _unit_loop(s, keep):
    q = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
    if math.isfinite(q) and q > 0:
        return [_round(s[k] / math.sqrt(q)) for k in range(3)]
    return keep


def raw_normals_loop(verts, tab):
    pos = _rows3(verts, tab["n_v"])
    out = np.zeros((len(tab["triangles"]), 3), F)
    for t, i in enumerate(tab["triangles"].tolist()):
        if not (_finite(pos[i[0]]) and _finite(pos[i[1]]) and _finite(pos[i[2]])):
            continue
        p = [[float(pos[i[k], a]) for a in range(3)] for k in range(3)]
        e1 = [p[1][a] - p[0][a] for a in range(3)]
        e2 = [p[2][a] - p[0][a] for a in range(3)]
        s = [(e1[1] * e2[2]) - (e1[2] * e2[1]), (e1[2] * e2[0]) - (e1[0] * e2[2]), (e1[0] * e2[1]) - (e1[1] * e2[0])]
        out[t] = _unit_loop(s, [F(0), F(0), F(0)])
    return out


def normal_pass_loop(nrm, tab, threshold):
    n = _rows3(nrm, len(tab["triangles"]), "one normal per triangle")
    out = n.copy()
    rows, T = tab["rows"], float(threshold)
    for t, (a, b, c) in enumerate(tab["triangles"].tolist()):
        nt = [float(x) for x in n[t]]
        if not _finite(nt) or nt == [0.0, 0.0, 0.0]:
            continue
        s = [0.0, 0.0, 0.0]
        for j in sorted(set(rows[a]) | set(rows[b]) | set(rows[c])):
            nj = [float(x) for x in n[j]]
            if not _finite(nj):
                continue
            d = (nt[0] * nj[0] + nt[1] * nj[1]) + nt[2] * nj[2]
            if not (math.isfinite(d) and d > T):
                continue
            w = (d - T) * (d - T)
            for k in range(3):
                s[k] = s[k] + w * nj[k]
        out[t] = _unit_loop(s, out[t].copy())
    return out


def vertex_pass_loop(verts, nrm, tab):
    pos = _rows3(verts, tab["n_v"])
    tri = tab["triangles"].tolist()
    N = _rows3(nrm, len(tri), "one normal per triangle")
    out = pos.copy()
    fin = [_finite(r) for r in pos]
    for v in range(len(pos)):
        if not fin[v]:
            continue
        x = [float(a) for a in pos[v]]
        s, m = [0.0, 0.0, 0.0], 0
        for t in sorted(set(tab["rows"][v])):
            Nt = [float(a) for a in N[t]]
            i = tri[t]
            if not _finite(Nt) or Nt == [0.0, 0.0, 0.0] or not (fin[i[0]] and fin[i[1]] and fin[i[2]]):
                continue
            e = [((float(pos[i[0], k]) + float(pos[i[1], k])) + float(pos[i[2], k])) / 3.0 - x[k] for k in range(3)]
            dd = (Nt[0] * e[0] + Nt[1] * e[1]) + Nt[2] * e[2]
            for k in range(3):
                s[k] = s[k] + Nt[k] * dd
            m += 1
        if m:
            out[v] = [_round(x[k] + s[k] / float(m)) for k in range(3)]
    return out


def denoise_loop(verts, triangles, normal_iterations=5, vertex_iterations=10, threshold=0.4, tab=None):
    pos = _rows3(verts)
    tab = face_table_loop(triangles, len(pos)) if tab is None else tab
    n = raw_normals_loop(pos, tab)
    for _ in range(normal_iterations):
        n = normal_pass_loop(n, tab, threshold)
    out = pos.copy()
    for _ in range(vertex_iterations):
        out = vertex_pass_loop(out, n, tab)
    return out, n


def same_table(a, b):
    """the names of the entries in which two face tables differ in a byte"""
    bad = [k for k in ("offsets", "faces") if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    return bad + (["counts"] if a["counts"] != b["counts"] else [])
