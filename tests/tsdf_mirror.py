"""numpy restatement of the TSDF volume's contract (include/rgbid_tsdf.h): the judge of csrc/kernels_tsdf.hip.
Every float32 value is formed by np.float32 operations in exactly the order of the header (no `@`, no fused operation); counts, colour
sums and every decision are integers and booleans.  `integrate` and `extract` are vectorised over the voxels; `integrate_loop` and
`extract_loop` are the plain scalar loops of the same contract that the CPU tests hold them against."""
import numpy as np

from tests.render_mirror import one_nan, pose_cw, rot_row

F = np.float32
MAX_W = 65535
TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))   # axis orders xyz xzy yxz yzx zxy zyx
# SWAP[tetrahedron][case]: the rows of that case have their last two entries swapped (derive_swap() re-derives it from the orientation rule)
SWAP = np.array([[0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0],
                 [0, 1, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0],
                 [0, 1, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0],
                 [0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0],
                 [0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0],
                 [0, 1, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0]], np.uint8)


def offset(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def case_rows(m):
    """the unswapped rows of case m (bit u set: vertex u of the tetrahedron is inside): a list of rows of three edges (u, v), u < v"""
    ins = [u for u in range(4) if m >> u & 1]
    outs = [u for u in range(4) if not m >> u & 1]
    e = lambda u, v: (min(u, v), max(u, v))
    if len(ins) == 1:
        return [tuple(e(ins[0], o) for o in outs)]
    if len(ins) == 3:
        return [tuple(e(i, outs[0]) for i in ins)]
    if len(ins) == 2:
        (a, b), (c, d) = ins, outs
        return [(e(a, c), e(a, d), e(b, d)), (e(a, c), e(b, d), e(b, c))]
    return []


def row_fails(t, m, row):
    """the orientation rule of step 12 for one unswapped row: every cut at its edge's midpoint, exact in small integers (doubled)"""
    P = [np.array(offset(c), np.int64) for c in TETS[t]]
    M = [P[u] + P[v] for u, v in row]
    u, v = row[0]
    p_in, p_out = (P[u], P[v]) if m >> u & 1 else (P[v], P[u])
    return int(np.dot(np.cross(M[1] - M[0], M[2] - M[0]), p_out - p_in)) < 0


def derive_swap():
    """SWAP from the rule; asserts that a case's rows agree, so that the swap is a property of (tetrahedron, case)"""
    s = np.zeros((6, 16), np.uint8)
    for t in range(6):
        for m in range(16):
            fails = {row_fails(t, m, row) for row in case_rows(m)}
            assert len(fails) <= 1, (t, m)
            s[t, m] = bool(fails and fails.pop())
    return s


def case_triangles(t, m):
    """the rows of (tetrahedron, case) after the swap, every edge as (corner of its lower vertex, offset code to the other)"""
    out = []
    for row in case_rows(m):
        row = (row[0], row[2], row[1]) if SWAP[t, m] else row
        out.append(tuple((TETS[t][u], TETS[t][v] - TETS[t][u]) for u, v in row))
    return out


class Volume:
    """shape and state: D float32, W, Cn uint32 [nz, ny, nx], rgb uint32 [3, nz, ny, nx]"""

    def __init__(self, nx, ny, nz, origin, voxel, trunc, colour=True):
        self.nx, self.ny, self.nz = int(nx), int(ny), int(nz)
        self.origin = np.asarray(origin, F).reshape(3)
        self.voxel, self.trunc, self.colour = F(voxel), F(trunc), colour
        self.reset()

    def reset(self):
        s = (self.nz, self.ny, self.nx)
        self.D, self.W, self.Cn, self.rgb = np.zeros(s, F), np.zeros(s, np.uint32), np.zeros(s, np.uint32), np.zeros((3,) + s, np.uint32)

    @property
    def shape(self):
        return (self.nz, self.ny, self.nx)

    @property
    def n(self):
        return self.nx * self.ny * self.nz

    def centres(self):
        """-> x [nx], y [ny], z [nz]: o + (float)i voxel"""
        o = self.origin
        return tuple(o[a] + np.arange(n, dtype=F) * self.voxel for a, n in enumerate((self.nx, self.ny, self.nz)))

    def counts(self):
        return self.W | (self.Cn << np.uint32(16))

    def set_state(self, D, counts, rgb=None):
        c = np.asarray(counts, np.uint32).reshape(self.shape)
        self.D = np.array(D, F).reshape(self.shape)
        self.W, self.Cn = c & np.uint32(0xFFFF), c >> np.uint32(16)
        self.rgb = np.zeros((3,) + self.shape, np.uint32) if rgb is None else np.array(rgb, np.uint32).reshape((3,) + self.shape)

    def state_bytes(self):
        return self.D.tobytes(), self.counts().tobytes(), self.rgb.tobytes()


def measured_depth(m):
    """step 5 for an array of inverse depths: -> (measured, z_m)"""
    m = np.asarray(m, F)
    with np.errstate(all="ignore"):
        zm = F(1) / m
        ok = np.isfinite(m) & (m > 0) & np.isfinite(zm)
    return ok, zm


def integrate(vol, planes, colours, R, t, K, z_min=0.05, z_max=20.0):
    """steps 1 - 8: planes [V][rows, cols] float32; colours None or [V] of None / uint8 [rows, cols, 3]; world poses R [V, 3, 3], t [V, 3]"""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3); t = np.asarray(t, np.float64).reshape(-1, 3)
    fx, fy, cx, cy = (F(v) for v in K)
    cxs, cys, czs = vol.centres()
    x, y, z = cxs[None, None, :], cys[None, :, None], czs[:, None, None]
    D, W, Cn, rgb = vol.D.reshape(-1), vol.W.reshape(-1), vol.Cn.reshape(-1), vol.rgb.reshape(3, -1)
    for v in range(len(R)):
        m = pose_cw(R[v], t[v])
        plane = np.asarray(planes[v], F)
        rows, cols = plane.shape
        with np.errstate(all="ignore"):
            X = rot_row(m[0:3], x, y, z) + m[9]
            Y = rot_row(m[3:6], x, y, z) + m[10]
            Z = rot_row(m[6:9], x, y, z) + m[11]
            ok = np.isfinite(Z) & (Z >= F(z_min)) & (Z <= F(z_max))
            pu = np.floor((fx * (X / Z) + cx) + F(0.5))
            pv = np.floor((fy * (Y / Z) + cy) + F(0.5))
            ok &= (pu >= F(0)) & (pu <= F(cols - 1)) & (pv >= F(0)) & (pv <= F(rows - 1))
        assert X.dtype == Z.dtype == pu.dtype == F and Z.shape == vol.shape
        i = np.nonzero(ok.reshape(-1))[0]
        iu, iv, Zi = pu.reshape(-1)[i].astype(np.int64), pv.reshape(-1)[i].astype(np.int64), Z.reshape(-1)[i]
        meas, zm = measured_depth(plane[iv, iu])
        with np.errstate(all="ignore"):
            s = zm - Zi
            take = meas & ~(s < -vol.trunc) & (W[i] < MAX_W)
        i, iu, iv, s = i[take], iu[take], iv[take], s[take]
        d = np.minimum(s, vol.trunc)
        w = W[i].astype(F)
        with np.errstate(all="ignore"):                      # a D that is not finite, or a huge one, is walked like any other
            D[i] = (D[i] * w + d) / (w + F(1))
        W[i] += np.uint32(1)
        if vol.colour and colours is not None and colours[v] is not None:
            c = np.abs(s) <= vol.trunc
            c &= Cn[i] < MAX_W
            col = np.asarray(colours[v], np.uint8).reshape(rows, cols, 3)
            for ch in range(3):
                rgb[ch, i[c]] += col[iv[c], iu[c], ch].astype(np.uint32)
            Cn[i[c]] += np.uint32(1)
    assert D.dtype == F
    return vol


def integrate_loop(vol, planes, colours, R, t, K, z_min, z_max):
    """steps 1 - 8 as a scalar loop over voxels and views"""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3); t = np.asarray(t, np.float64).reshape(-1, 3)
    fx, fy, cx, cy = (F(v) for v in K)
    ms = [pose_cw(R[v], t[v]) for v in range(len(R))]
    o, h, tr = vol.origin, vol.voxel, vol.trunc
    with np.errstate(all="ignore"):
        for k in range(vol.nz):
            for j in range(vol.ny):
                for i in range(vol.nx):
                    x, y, z = F(o[0] + F(F(i) * h)), F(o[1] + F(F(j) * h)), F(o[2] + F(F(k) * h))
                    for v, m in enumerate(ms):
                        plane = planes[v]
                        rows, cols = plane.shape
                        X = F(F(F(m[0] * x) + F(m[1] * y)) + F(m[2] * z)) + m[9]
                        Y = F(F(F(m[3] * x) + F(m[4] * y)) + F(m[5] * z)) + m[10]
                        Z = F(F(F(m[6] * x) + F(m[7] * y)) + F(m[8] * z)) + m[11]
                        if not (F(z_min) <= Z <= F(z_max)):
                            continue
                        pu = np.floor(F(F(fx * F(X / Z)) + cx) + F(0.5))
                        pv = np.floor(F(F(fy * F(Y / Z)) + cy) + F(0.5))
                        if not (0 <= pu <= cols - 1 and 0 <= pv <= rows - 1):
                            continue
                        pu, pv = int(pu), int(pv)
                        iD = F(plane[pv, pu])
                        if not (np.isfinite(iD) and iD > 0):
                            continue
                        zm = F(F(1) / iD)
                        if not np.isfinite(zm):
                            continue
                        s = F(zm - Z)
                        if s < -tr or vol.W[k, j, i] == MAX_W:
                            continue
                        d = min(s, tr)
                        w = F(vol.W[k, j, i])
                        vol.D[k, j, i] = F(F(F(vol.D[k, j, i] * w) + d) / F(w + F(1)))
                        vol.W[k, j, i] += 1
                        if vol.colour and colours is not None and colours[v] is not None and abs(s) <= tr and vol.Cn[k, j, i] < MAX_W:
                            vol.rgb[:, k, j, i] += np.asarray(colours[v]).reshape(rows, cols, 3)[pv, pu].astype(np.uint32)
                            vol.Cn[k, j, i] += 1
    return vol


def _means(vol):
    """step 11: -> (has [n] bool, mean float32 [3, n])"""
    Cn = vol.Cn.reshape(-1).astype(np.uint64)
    has = (Cn > 0) & bool(vol.colour)
    s = vol.rgb.reshape(3, -1).astype(np.uint64)
    mean = np.minimum((2 * s + Cn) // np.maximum(2 * Cn, 1), 255)
    return has, mean.astype(F)


def extract(vol, min_weight=1):
    """steps 9 - 12: -> (vertices float32 [nv, 3], colours uint8 [nv, 3], triangles uint32 [nt, 3])"""
    nx, ny, nz, n = vol.nx, vol.ny, vol.nz, vol.n
    valid = vol.W >= min_weight
    with np.errstate(invalid="ignore"):
        inside = valid & (vol.D < 0)
    lin = np.arange(n, dtype=np.int64).reshape(vol.shape)
    act = np.zeros((n, 7), bool)
    for c in range(1, 8):
        dx, dy, dz = offset(c)
        P = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        Q = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        a = valid[P] & valid[Q] & (inside[P] != inside[Q])
        act[lin[P][a], c - 1] = True
    flat = act.reshape(-1)
    vidx = np.cumsum(flat, dtype=np.int64) - 1
    e = np.nonzero(flat)[0]
    p, c = e // 7, e % 7 + 1
    q = p + (c & 1) + ((c >> 1) & 1) * nx + ((c >> 2) & 1) * nx * ny
    ins = inside.reshape(-1)
    a, b = np.where(ins[p], p, q), np.where(ins[p], q, p)
    D = vol.D.reshape(-1)
    with np.errstate(all="ignore"):
        tt = D[a] / (D[a] - D[b])
        verts = np.empty((len(e), 3), F)
        for ax, (cen, div, mod) in enumerate(zip(vol.centres(), (1, nx, nx * ny), (nx, ny, nz))):
            pa, pb = cen[a // div % mod], cen[b // div % mod]
            verts[:, ax] = pa + tt * (pb - pa)
        has, mean = _means(vol)
        cols = np.zeros((len(e), 3), np.uint8)
        both = has[a] & has[b]
        for ch in range(3):
            ca, cb = mean[ch, a], mean[ch, b]
            mix = np.fmin(np.fmax(np.floor((ca + tt * (cb - ca)) + F(0.5)), F(0)), F(255))
            mix = np.where(np.isnan(mix), F(0), mix)
            cols[:, ch] = np.where(both, mix, np.where(has[a], ca, np.where(has[b], cb, F(0)))).astype(np.uint8)
    assert verts.dtype == F and tt.dtype == F
    verts = one_nan(verts)                                   # step 10: every NaN component has the one bit pattern
    # triangles: the cells whose 8 corners are valid, their 8-bit inside code, then per (tetrahedron, case) the table's rows
    C = (slice(0, nz - 1), slice(0, ny - 1), slice(0, nx - 1))
    allv = np.ones((nz - 1, ny - 1, nx - 1), bool)
    code = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for c in range(8):
        dx, dy, dz = offset(c)
        Q = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
        allv &= valid[Q]
        code |= inside[Q].astype(np.int64) << c
    cell = lin[C][allv]
    code = code[allv]
    keys, tris = [], []
    for t, tet in enumerate(TETS):
        m = sum(((code >> tet[u]) & 1) << u for u in range(4))
        for case in range(1, 15):
            sel = np.nonzero(m == case)[0]
            if not len(sel):
                continue
            for r, row in enumerate(case_triangles(t, case)):
                tri = np.empty((len(sel), 3), np.int64)
                for k, (corner, cd) in enumerate(row):
                    dx, dy, dz = offset(corner)
                    tri[:, k] = vidx[(cell[sel] + dx + dy * nx + dz * nx * ny) * 7 + cd - 1]
                    assert flat[(cell[sel] + dx + dy * nx + dz * nx * ny) * 7 + cd - 1].all()
                keys.append((sel * 6 + t) * 2 + r)
                tris.append(tri)
    if tris:
        order = np.argsort(np.concatenate(keys), kind="stable")
        tri = np.concatenate(tris)[order].astype(np.uint32)
    else:
        tri = np.zeros((0, 3), np.uint32)
    return verts, cols, tri


def extract_loop(vol, min_weight):
    """steps 9 - 12 as scalar loops -> (vertices, colours, triangles) as lists"""
    nx, ny, nz = vol.nx, vol.ny, vol.nz
    cen = vol.centres()
    valid = lambda i, j, k: vol.W[k, j, i] >= min_weight
    inside = lambda i, j, k: bool(valid(i, j, k) and vol.D[k, j, i] < 0)
    index, verts, cols = {}, [], []
    with np.errstate(all="ignore"):
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    for c in range(1, 8):
                        dx, dy, dz = offset(c)
                        qi, qj, qk = i + dx, j + dy, k + dz
                        if qi >= nx or qj >= ny or qk >= nz or not (valid(i, j, k) and valid(qi, qj, qk)):
                            continue
                        if inside(i, j, k) == inside(qi, qj, qk):
                            continue
                        index[(i, j, k, c)] = len(verts)
                        a, b = ((i, j, k), (qi, qj, qk)) if inside(i, j, k) else ((qi, qj, qk), (i, j, k))
                        Da, Db = vol.D[a[2], a[1], a[0]], vol.D[b[2], b[1], b[0]]
                        tt = F(Da / F(Da - Db))
                        verts.append(one_nan([F(cen[x][a[x]] + F(tt * F(cen[x][b[x]] - cen[x][a[x]]))) for x in range(3)]))
                        mean = []
                        for e in (a, b):
                            cn = int(vol.Cn[e[2], e[1], e[0]])
                            mean.append([min((2 * int(vol.rgb[ch, e[2], e[1], e[0]]) + cn) // (2 * cn), 255) for ch in range(3)]
                                        if cn and vol.colour else None)
                        if mean[0] and mean[1]:
                            mix = [F(np.floor(F(F(F(ma) + F(tt * F(F(mb) - F(ma)))) + F(0.5)))) for ma, mb in zip(*mean)]
                            col = [0 if x != x else int(min(max(x, 0), 255)) for x in mix]          # a NaN gives 0
                        else:
                            col = mean[0] or mean[1] or [0, 0, 0]
                        cols.append(col)
    tris = []
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                corners = [(i + offset(c)[0], j + offset(c)[1], k + offset(c)[2]) for c in range(8)]
                if not all(valid(*p) for p in corners):
                    continue
                for t, tet in enumerate(TETS):
                    m = sum(int(inside(*corners[tet[u]])) << u for u in range(4))
                    for row in case_triangles(t, m):
                        tris.append([index[corners[corner] + (cd,)] for corner, cd in row])
    return verts, cols, tris


def mesh_topology(tri):
    """-> (undirected edges, the number of them in exactly two triangles, directed edges that occur more than once)"""
    tri = np.asarray(tri, np.int64)
    d = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    dk = d[:, 0] * (int(tri.max()) + 1 if len(tri) else 1) + d[:, 1]
    u = np.sort(d, axis=1)
    uk = u[:, 0] * (int(tri.max()) + 1 if len(tri) else 1) + u[:, 1]
    _, uc = np.unique(uk, return_counts=True)
    _, dc = np.unique(dk, return_counts=True)
    return len(uc), int((uc == 2).sum()), int((dc > 1).sum())


def signed_volume(verts, tri):
    v = np.asarray(verts, np.float64)[np.asarray(tri, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def sphere_state(vol, centre, radius):
    """D = min(|p - c| - r, trunc), every W = 1: the state of the sphere tests"""
    x, y, z = vol.centres()
    c = np.asarray(centre, F)
    dist = np.sqrt((x[None, None, :] - c[0]) ** 2 + (y[None, :, None] - c[1]) ** 2 + (z[:, None, None] - c[2]) ** 2).astype(F)
    return np.minimum(dist - F(radius), vol.trunc).astype(F), np.ones(vol.shape, np.uint32)
