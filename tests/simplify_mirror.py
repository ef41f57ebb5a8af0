"""numpy restatement of the vertex clustering contract (include/rgbid_simplify.h), steps 1 - 6, stated twice:
`simplify` vectorised (np.unique for the clusters and the triples, np.add.at for the sums, which adds one element after the other in
index order; np.add.reduceat and np.sum are pairwise over eight elements and more and would not do) and `simplify_loop`, plain scalar
loops over dictionaries.  Both are written from the contract, not from the kernels.  Only integers decide; float32 is numpy's float32
arithmetic, one rounding per operation; the sums are Python / numpy doubles."""
import math

import numpy as np

F, U32 = np.float32, np.uint32
NO_CLUSTER = 0xFFFFFFFF
COUNTS = ("participating", "clusters", "lost", "collapsed", "duplicate", "kept")


def _inputs(vertices, triangles, cell):
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    tri = np.ascontiguousarray(np.asarray(triangles).reshape(-1, 3)).astype(np.int64)
    if len(tri) and (tri.min() < 0 or tri.max() >= len(v)):
        raise ValueError("a triangle names a vertex that does not exist")      # step 1: the mesh is refused
    cell = np.broadcast_to(np.asarray(cell, F), (3,)).astype(F)
    if not (np.isfinite(cell).all() and (cell > 0).all()):
        raise ValueError("cell: finite and > 0")
    return v, tri, cell


def form_grid(lo, hi, cell):
    """section 12's grid in float32 from the box of the participating vertices -> (inv float32 [3], min_b, div_b as Python integers)"""
    inv = F(1.0) / cell
    flo, fhi = np.floor(lo * inv), np.floor(hi * inv)
    if not ((flo >= -2.0**31).all() and (flo < 2.0**31).all() and (fhi >= -2.0**31).all() and (fhi < 2.0**31).all()):
        raise ValueError("a bound of the grid leaves the int32 range")
    min_b = [int(x) for x in flo]
    div_b = [int(fhi[a]) - min_b[a] + 1 for a in range(3)]
    if div_b[0] * div_b[1] * div_b[2] >= 1 << 62:
        raise ValueError("2^62 cells or more")
    return inv, min_b, div_b


# ---- the vectorised statement -----------------------------------------------------------------------------------------------------------
def simplify(vertices, triangles, cell, colours=None, normals=None, keep_duplicates=False):
    """-> dict(grid int64 [6], counts dict, cluster_of uint32 [n_v], vertices float32 [C, 3], colours uint8 [C, 3] or None, normals float32
    [C, 3] or None, members uint32 [C], triangles uint32 [kept, 3], classes uint8 [n_t]: 0 lost, 1 collapsed, 2 duplicate, 3 kept)"""
    v, tri, cell = _inputs(vertices, triangles, cell)
    n_v, n_t = len(v), len(tri)
    part = np.isfinite(v).all(1)
    who = np.nonzero(part)[0]                                  # ascending vertex index: the member order
    cluster_of = np.full(n_v, NO_CLUSTER, np.int64)
    grid = np.zeros(6, np.int64)
    n_c = 0
    if len(who):
        p = v[who]
        inv, min_b, div_b = form_grid(p.min(0), p.max(0), cell)
        grid[:] = min_b + div_b
        ijk = (np.floor(p * inv) - np.array(min_b, F)).astype(np.int64)      # one float multiply, floor, one float subtraction
        key = ijk[:, 0] + ijk[:, 1] * div_b[0] + ijk[:, 2] * (div_b[0] * div_b[1])   # below the 2^62 cells of the grid: int64 holds it
        uniq, inverse = np.unique(key, return_inverse=True)
        n_c = len(uniq)
        cluster_of[who] = inverse.reshape(-1)
    cl = cluster_of[who]
    members = np.bincount(cl, minlength=n_c).astype(np.int64)
    sums = np.zeros((n_c, 3), np.float64)
    for a in range(3):
        np.add.at(sums[:, a], cl, v[who, a].astype(np.float64))              # sequential adds in member order
    out_v = (sums / members[:, None].astype(np.float64)).astype(F)
    out_c = out_n = None
    if colours is not None:
        col = np.ascontiguousarray(colours, np.uint8).reshape(-1, 3)[who].astype(np.int64)
        csum = np.zeros((n_c, 3), np.int64)
        np.add.at(csum, cl, col)
        out_c = ((2 * csum + members[:, None]) // (2 * members[:, None])).astype(np.uint8)
    if normals is not None:
        nrm = np.ascontiguousarray(normals, F).reshape(-1, 3)[who]
        ok = np.isfinite(nrm).all(1)
        s = np.zeros((n_c, 3), np.float64)
        for a in range(3):
            np.add.at(s[:, a], cl[ok], nrm[ok, a].astype(np.float64))
        has = np.bincount(cl[ok], minlength=n_c) > 0
        with np.errstate(all="ignore"):
            q = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
            good = has & (q != 0) & np.isfinite(q)
            out_n = np.where(good[:, None], s / np.sqrt(q)[:, None], 0.0).astype(F)
    # step 5
    t = cluster_of[tri] if n_t else np.zeros((0, 3), np.int64)
    classes = np.full(n_t, 3, np.uint8)
    lost = (t == NO_CLUSTER).any(1)
    collapsed = ~lost & ((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2]))
    classes[lost], classes[collapsed] = 0, 1
    cand = np.nonzero(~lost & ~collapsed)[0]
    if not keep_duplicates and len(cand):
        _, first = np.unique(np.sort(t[cand], 1), axis=0, return_index=True)  # the first occurrence of every set of three clusters
        dup = np.ones(len(cand), bool)
        dup[first] = False
        classes[cand[dup]] = 2
    kept = t[classes == 3].astype(U32).reshape(-1, 3)
    counts = dict(participating=int(len(who)), clusters=int(n_c), lost=int((classes == 0).sum()), collapsed=int((classes == 1).sum()),
                  duplicate=int((classes == 2).sum()), kept=len(kept))
    return dict(grid=grid, counts=counts, cluster_of=cluster_of.astype(U32), vertices=out_v.reshape(-1, 3), colours=out_c, normals=out_n,
                members=members.astype(U32), triangles=kept, classes=classes)


# ---- the second statement: scalar loops ----------------------------------------------------------------------------------------------------
def simplify_loop(vertices, triangles, cell, colours=None, normals=None, keep_duplicates=False):
    """the same dictionary from plain loops, one vertex and one triangle at a time"""
    v, tri, cell = _inputs(vertices, triangles, cell)
    n_v, n_t = len(v), len(tri)
    fin = lambda row: all(math.isfinite(float(x)) for x in row)
    who = [i for i in range(n_v) if fin(v[i])]
    grid, cells = [0] * 6, {}
    if who:
        lo = [min(v[i, a] for i in who) for a in range(3)]
        hi = [max(v[i, a] for i in who) for a in range(3)]
        inv = [F(1.0) / cell[a] for a in range(3)]
        min_b = [int(math.floor(F(lo[a] * inv[a]))) for a in range(3)]
        div_b = [int(math.floor(F(hi[a] * inv[a]))) - min_b[a] + 1 for a in range(3)]
        grid = min_b + div_b
        for i in who:                                          # ascending vertex index: a cell's list is in member order
            ijk = [int(F(F(math.floor(F(v[i, a] * inv[a]))) - F(min_b[a]))) for a in range(3)]
            cells.setdefault(ijk[0] + ijk[1] * div_b[0] + ijk[2] * div_b[0] * div_b[1], []).append(i)
    keys = sorted(cells)
    cluster_of = [NO_CLUSTER] * n_v
    out_v, out_c, out_n, members = [], [], [], []
    col = None if colours is None else np.ascontiguousarray(colours, np.uint8).reshape(-1, 3)
    nrm = None if normals is None else np.ascontiguousarray(normals, F).reshape(-1, 3)
    for c, k in enumerate(keys):
        s, cs, ns, any_normal = [0.0] * 3, [0] * 3, [0.0] * 3, False
        for i in cells[k]:
            cluster_of[i] = c
            for a in range(3):
                s[a] += float(v[i, a])
                if col is not None:
                    cs[a] += int(col[i, a])
            if nrm is not None and fin(nrm[i]):
                any_normal = True
                for a in range(3):
                    ns[a] += float(nrm[i, a])
        n = len(cells[k])
        members.append(n)
        out_v.append([F(s[a] / float(n)) for a in range(3)])
        out_c.append([(2 * cs[a] + n) // (2 * n) for a in range(3)])
        q = (ns[0] * ns[0] + ns[1] * ns[1]) + ns[2] * ns[2]     # Python floats are doubles; a product that overflows is inf
        if any_normal and q != 0.0 and math.isfinite(q):
            out_n.append([F(ns[a] / math.sqrt(q)) for a in range(3)])
        else:
            out_n.append([F(0.0)] * 3)
    classes, kept, seen = [], [], set()
    for row in tri:
        t = [cluster_of[int(i)] for i in row]
        if NO_CLUSTER in t:
            classes.append(0)
        elif t[0] == t[1] or t[1] == t[2] or t[0] == t[2]:
            classes.append(1)
        elif not keep_duplicates and tuple(sorted(t)) in seen:
            classes.append(2)
        else:
            seen.add(tuple(sorted(t)))
            classes.append(3)
            kept.append(t)
    counts = dict(participating=len(who), clusters=len(keys), lost=classes.count(0), collapsed=classes.count(1), duplicate=classes.count(2),
                  kept=len(kept))
    return dict(grid=np.array(grid, np.int64), counts=counts, cluster_of=np.array(cluster_of, np.int64).astype(U32),
                vertices=np.array(out_v, F).reshape(-1, 3), colours=None if col is None else np.array(out_c, np.uint8).reshape(-1, 3),
                normals=None if nrm is None else np.array(out_n, F).reshape(-1, 3), members=np.array(members, U32),
                triangles=np.array(kept, np.int64).astype(U32).reshape(-1, 3), classes=np.array(classes, np.uint8))


def same(a, b):
    """the names of the entries in which two results differ in a byte"""
    bad = [k for k in ("grid", "cluster_of", "vertices", "colours", "normals", "members", "triangles", "classes")
           if (a[k] is None) != (b[k] is None) or (a[k] is not None and (a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()))]
    return bad + (["counts"] if a["counts"] != b["counts"] else [])
