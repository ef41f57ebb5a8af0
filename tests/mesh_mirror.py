"""numpy restatement of the mesh component contract (include/rgbid_mesh.h), steps 1 - 5: `label`, `select` and `emit`
vectorised (a min-label scatter with np.minimum.at plus pointer jumping, to a fixpoint), and `label_loop` / `filter_loop`, a plain
sequential union-find over the same contract as the independent second statement.  Only integers decide; attribute bytes are copied."""
import numpy as np

U32 = np.uint32


def _mesh(triangles, n_vertices):
    tri = np.ascontiguousarray(np.asarray(triangles).reshape(-1, 3)).astype(np.int64)
    n_v = int(n_vertices)
    if len(tri) and (tri.min() < 0 or tri.max() >= n_v):
        raise ValueError("a triangle names a vertex that does not exist")      # step 1: the mesh is refused
    return tri, n_v


def roots(triangles, n_vertices, count_rounds=False):
    """step 2: -> root int64 [n_v], the smallest vertex index of every vertex's component"""
    tri, n_v = _mesh(triangles, n_vertices)
    lab = np.arange(n_v, dtype=np.int64)
    rounds = 0
    while True:
        rounds += 1
        before = lab.copy()
        if len(tri):
            m = lab[tri].min(1)                      # the smallest label a triangle sees goes to the labels' own vertices: a hook
            for k in range(3):
                np.minimum.at(lab, lab[tri[:, k]], m)
                np.minimum.at(lab, tri[:, k], m)
        while True:                                  # pointer jumping: lab[v] <= v, so it ends at a fixpoint
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
        if np.array_equal(lab, before):
            return (lab, rounds) if count_rounds else lab


def _table(root, tri, n_v):
    is_root = root == np.arange(n_v)
    rts = np.nonzero(is_root)[0]
    number = np.cumsum(is_root) - 1                  # per root: its rank
    nverts = np.bincount(root, minlength=n_v)[rts] if n_v else np.zeros(0, np.int64)
    ntris = np.bincount(root[tri[:, 0]], minlength=n_v)[rts] if len(tri) else np.zeros(len(rts), np.int64)
    table = np.stack([rts, nverts, ntris], 1).astype(U32).reshape(-1, 3)
    labels = number[root].astype(U32) if n_v else np.zeros(0, U32)
    return table, labels


def label(triangles, n_vertices):
    """steps 1 - 3: -> (table uint32 [C, 3] = root, vertices, triangles; labels uint32 [n_v])"""
    tri, n_v = _mesh(triangles, n_vertices)
    return _table(roots(tri, n_v), tri, n_v)


def select(table, min_triangles=1, mask=None):
    """step 4: -> keep bool [C]"""
    keep = table[:, 2].astype(np.int64) >= int(min_triangles)
    if mask is not None:
        mask = np.asarray(mask, np.uint8).reshape(-1)
        assert len(mask) == len(table)
        keep = keep & (mask != 0)
    return keep


def largest_mask(table, k):
    """uint8 [C]: 1 for the k components first in the order (triangles descending, root ascending)"""
    order = np.lexsort((table[:, 0].astype(np.int64), -table[:, 2].astype(np.int64)))
    mask = np.zeros(len(table), np.uint8)
    mask[order[:int(k)]] = 1
    return mask


def emit(triangles, labels, keep, vertices, colours=None, normals=None):
    """step 5: -> dict(vertices, colours, normals, old_index, triangles, components): the kept part, attributes copied as bytes"""
    tri = np.ascontiguousarray(np.asarray(triangles).reshape(-1, 3)).astype(np.int64)
    labels = np.asarray(labels, np.int64)
    keep = np.asarray(keep, bool)
    kv = keep[labels] if len(labels) else np.zeros(0, bool)
    old = np.nonzero(kv)[0]
    remap = np.cumsum(kv) - 1
    kt = kv[tri[:, 0]] if len(tri) else np.zeros(0, bool)
    words = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).reshape(-1, 3).view(U32)[old].view(np.float32)
    return dict(vertices=words(vertices), colours=None if colours is None else np.ascontiguousarray(colours, np.uint8).reshape(-1, 3)[old],
                normals=words(normals), old_index=old.astype(U32), triangles=remap[tri[kt]].astype(U32).reshape(-1, 3),
                components=int(keep.sum()))


def filter_mesh(triangles, n_vertices, vertices, colours=None, normals=None, min_triangles=1, mask=None, largest=None):
    """steps 1 - 5 in one: -> emit's dict with table and labels added"""
    table, labels = label(triangles, n_vertices)
    if largest is not None:
        assert mask is None
        mask = largest_mask(table, largest)
    out = emit(triangles, labels, select(table, min_triangles, mask), vertices, colours, normals)
    out.update(table=table, labels=labels)
    return out


# ---- the second statement: a sequential union-find, one triangle and one vertex at a time -----------------------------------------------
def label_loop(triangles, n_vertices):
    tri = [[int(x) for x in t] for t in np.asarray(triangles).reshape(-1, 3)]
    n_v = int(n_vertices)
    for t in tri:
        if not all(0 <= i < n_v for i in t):
            raise ValueError("a triangle names a vertex that does not exist")
    parent = list(range(n_v))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in tri:
        for u, v in ((a, b), (b, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    root = [find(v) for v in range(n_v)]
    number, table = {}, []
    for v in range(n_v):
        if root[v] == v:
            number[v] = len(table)
            table.append([v, 0, 0])
    for v in range(n_v):
        table[number[root[v]]][1] += 1
    for t in tri:
        table[number[root[t[0]]]][2] += 1
    return table, [number[root[v]] for v in range(n_v)]


def filter_loop(triangles, n_vertices, min_triangles=1, mask=None):
    """-> (old indices of the kept vertices, the kept triangles renumbered, kept components) as lists"""
    table, labels = label_loop(triangles, n_vertices)
    keep = [row[2] >= min_triangles and (mask is None or mask[c] != 0) for c, row in enumerate(table)]
    old, remap = [], {}
    for v in range(int(n_vertices)):
        if keep[labels[v]]:
            remap[v] = len(old)
            old.append(v)
    tris = [[remap[int(i)] for i in t] for t in np.asarray(triangles).reshape(-1, 3) if keep[labels[int(t[0])]]]
    return old, tris, sum(keep)
