"""numpy restatement of steps 13 - 23 of the TSDF volume's contract (include/rgbid_tsdf_raycast.h): the judge of
k_tsdf_raycast and of the vertex normals in csrc/kernels_tsdf.hip.  Every float32 value is formed by np.float32 operations in exactly the
order of the header; integers and comparisons decide.  `raycast` and `vertex_normals` are vectorised over pixels and edges and visit every
n (no clipping); `raycast_loop` and `normals_loop` are the plain scalar loops of the same contract that the CPU tests hold them against."""
import numpy as np

from tests.render_mirror import NAN_BITS, one_nan
from tests.tsdf_mirror import _means, offset

F = np.float32
MAX_STEPS = 65536


def pose_wc(R, t):
    """step 13: world pose (double) -> R00 .. R22, tx, ty, tz as float32"""
    with np.errstate(over="ignore"):
        return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)]).astype(F)


def depth_of(n, z_min, step):
    return F(z_min) + F(n) * F(step)


def last_step(z_min, z_max, step):
    """step 15: the largest n <= MAX_STEPS with Z_m <= z_max for every m <= n"""
    n = 0
    while n < MAX_STEPS and depth_of(n + 1, z_min, step) <= F(z_max):
        n += 1
    return n


def lerp(a, b, f):
    return a + f * (b - a)


def trilinear(d, fx, fy, fz):
    """step 16's value of the corner values d[i + 2 j + 4 k]"""
    ly0 = lerp(lerp(d[0], d[1], fx), lerp(d[2], d[3], fx), fy)
    ly1 = lerp(lerp(d[4], d[5], fx), lerp(d[6], d[7], fx), fy)
    return lerp(ly0, ly1, fz)


def gradient(d, fx, fy, fz):
    lx00, lx10, lx01, lx11 = lerp(d[0], d[1], fx), lerp(d[2], d[3], fx), lerp(d[4], d[5], fx), lerp(d[6], d[7], fx)
    gx = lerp(lerp(d[1] - d[0], d[3] - d[2], fy), lerp(d[5] - d[4], d[7] - d[6], fy), fz)
    gy = lerp(lx10 - lx00, lx11 - lx01, fz)
    gz = lerp(lx01, lx11, fy) - lerp(lx00, lx10, fy)
    return gx, gy, gz


def corner_offsets(vol):
    return [dx + dy * vol.nx + dz * vol.nx * vol.ny for dx, dy, dz in (offset(c) for c in range(8))]


def cell(vol, gx, gy, gz, min_weight):
    """step 15 for arrays of positions -> (defined, base: the linear index of corner 000 (0 where out of range), fx_, fy_, fz_)"""
    with np.errstate(invalid="ignore"):
        i0, j0, k0 = np.floor(gx), np.floor(gy), np.floor(gz)
        ok = ((i0 >= 0) & (i0.astype(np.float64) <= vol.nx - 2) & (j0 >= 0) & (j0.astype(np.float64) <= vol.ny - 2)
              & (k0 >= 0) & (k0.astype(np.float64) <= vol.nz - 2))                    # the float against the integer, exactly; NaN fails
        fx_, fy_, fz_ = gx - i0, gy - j0, gz - k0
    assert i0.dtype == fx_.dtype == F
    ii, jj, kk = (np.where(ok, v, F(0)).astype(np.int64) for v in (i0, j0, k0))
    base = (kk * vol.ny + jj) * vol.nx + ii
    W = vol.W.reshape(-1)
    defined = ok.copy()
    for o in corner_offsets(vol):
        defined &= W[base + o] >= min_weight
    return defined, base, fx_, fy_, fz_


def rays(vol, m, K, rows, cols):
    """step 14 for every pixel of a view -> (ax, ay, az scalars; bx, by, bz float32 [rows cols])"""
    fx, fy, cx, cy = (F(v) for v in K)
    pu, pv = np.meshgrid(np.arange(cols, dtype=F), np.arange(rows, dtype=F))
    dx, dy = ((pu - cx) / fx).reshape(-1), ((pv - cy) / fy).reshape(-1)
    with np.errstate(all="ignore"):
        a = [(m[9 + i] - vol.origin[i]) / vol.voxel for i in range(3)]
        b = [((m[3 * i] * dx + m[3 * i + 1] * dy) + m[3 * i + 2]) / vol.voxel for i in range(3)]
    assert all(x.dtype == F for x in a + b)
    return a, b


def shade_hit(vol, m, base, fx_, fy_, fz_, defined):
    """steps 19 and 20 for the re-samples (arrays over the hit pixels) -> (normal float32 [3, h], colour uint8 [h, 3])"""
    offs = corner_offsets(vol)
    D = vol.D.reshape(-1)
    d = [D[base + o] for o in offs]
    with np.errstate(all="ignore"):
        gx, gy, gz = gradient(d, fx_, fy_, fz_)
        L = np.sqrt((gx * gx + gy * gy) + gz * gz)
        ok = defined & (L > 0) & np.isfinite(L)
        nw = [gx / L, gy / L, gz / L]
        nc = np.stack([(m[i] * nw[0] + m[3 + i] * nw[1]) + m[6 + i] * nw[2] for i in range(3)])
    assert L.dtype == nc.dtype == F
    nc[:, ~ok] = np.nan
    has, mean = _means(vol)
    hs = np.stack([has[base + o] for o in offs])
    allc = hs.all(0)
    near = (fx_ >= F(0.5)).astype(np.int64) + 2 * (fy_ >= F(0.5)) + 4 * (fz_ >= F(0.5))
    near_idx = base + np.asarray(offs, np.int64)[near]
    col = np.zeros((len(base), 3), np.uint8)
    for ch in range(3):
        c = [mean[ch, base + o] for o in offs]
        with np.errstate(all="ignore"):
            mix = np.fmin(np.fmax(np.floor(trilinear(c, fx_, fy_, fz_) + F(0.5)), F(0)), F(255))
        mix = np.where(np.isnan(mix), F(0), mix)
        col[:, ch] = np.where(defined & allc, mix, np.where(defined & has[near_idx], mean[ch, near_idx], F(0))).astype(np.uint8)
    return nc, col


def raycast(vol, R, t, K, rows, cols, z_min, z_max, step, min_weight=1):
    """steps 13 - 21 -> dict(depth float32 [V, rows, cols], normal float32 [V, 3, rows, cols], colour uint8 [V, rows, cols, 3]) and, for
    the tests, hit_n int64 [V, rows, cols] (the n of the hit, -1 none), exit_n (the n of the exit, -1 none), redefined bool (the
    re-sample of a hit was defined)"""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3); t = np.asarray(t, np.float64).reshape(-1, 3)
    P = rows * cols
    offs = corner_offsets(vol)
    D = vol.D.reshape(-1)
    nl = last_step(z_min, z_max, step)
    out = {k: [] for k in ("depth", "normal", "colour", "hit_n", "exit_n", "redefined")}
    for v in range(len(R)):
        m = pose_wc(R[v], t[v])
        a, b = rays(vol, m, K, rows, cols)
        active = np.arange(P)
        prev = np.zeros(P, bool); f_prev = np.zeros(P, F)
        hit_n = np.full(P, -1, np.int64); exit_n = np.full(P, -1, np.int64); zs = np.full(P, np.nan, F)
        z_prev = F(0)
        for n in range(nl + 1):
            if not len(active):
                break
            Z = depth_of(n, z_min, step)
            with np.errstate(all="ignore"):
                g = [a[i] + Z * b[i][active] for i in range(3)]
                defined, base, fx_, fy_, fz_ = cell(vol, g[0], g[1], g[2], min_weight)
                f = trilinear([D[base + o] for o in offs], fx_, fy_, fz_)
                pair = defined & prev[active]
                fp = f_prev[active]
                hit = pair & (fp > 0) & (f <= 0)
                ext = pair & ~hit & ~(fp > 0) & (f > 0)
                tt = fp / (fp - f)
                z_hit = z_prev + tt * (Z - z_prev)
            assert f.dtype == z_hit.dtype == F
            hit_n[active[hit]] = n; zs[active[hit]] = z_hit[hit]
            exit_n[active[ext]] = n
            prev[active] = defined
            f_prev[active] = np.where(defined, f, F(0))
            z_prev = Z
            active = active[~(hit | ext)]
        h = np.nonzero(hit_n >= 0)[0]
        with np.errstate(all="ignore"):
            defined, base, fx_, fy_, fz_ = cell(vol, *[a[i] + zs[h] * b[i][h] for i in range(3)], min_weight)
        nc, col = shade_hit(vol, m, base, fx_, fy_, fz_, defined)
        depth = np.full(P, np.nan, F); depth[h] = zs[h]
        normal = np.full((3, P), np.nan, F); normal[:, h] = nc
        colour = np.zeros((P, 3), np.uint8); colour[h] = col
        redef = np.zeros(P, bool); redef[h] = defined
        out["depth"].append(one_nan(depth).reshape(rows, cols)); out["normal"].append(one_nan(normal).reshape(3, rows, cols))
        out["colour"].append(colour.reshape(rows, cols, 3)); out["hit_n"].append(hit_n.reshape(rows, cols))
        out["exit_n"].append(exit_n.reshape(rows, cols)); out["redefined"].append(redef.reshape(rows, cols))
    return {k: np.stack(x) for k, x in out.items()}


def _sample_loop(vol, gx, gy, gz, min_weight):
    """steps 15 and 16 for one position: None when undefined, else (corner indices (i, j, k) of 000, fx_, fy_, fz_, d[8])"""
    i0, j0, k0 = np.floor(gx), np.floor(gy), np.floor(gz)
    if not (0 <= i0 <= vol.nx - 2 and 0 <= j0 <= vol.ny - 2 and 0 <= k0 <= vol.nz - 2):
        return None
    i, j, k = int(i0), int(j0), int(k0)
    corners = [(i + dx, j + dy, k + dz) for dx, dy, dz in (offset(c) for c in range(8))]
    if any(vol.W[c[2], c[1], c[0]] < min_weight for c in corners):
        return None
    return corners, F(gx - i0), F(gy - j0), F(gz - k0), [F(vol.D[c[2], c[1], c[0]]) for c in corners]


def _l(a, b, f):
    return F(a + F(f * F(b - a)))


def _tri_loop(d, fx, fy, fz):
    return _l(_l(_l(d[0], d[1], fx), _l(d[2], d[3], fx), fy), _l(_l(d[4], d[5], fx), _l(d[6], d[7], fx), fy), fz)


def raycast_loop(vol, R, t, K, rows, cols, z_min, z_max, step, min_weight=1):
    """steps 13 - 21 as scalar loops over views, pixels and samples -> (depth, normal, colour) as raycast's arrays"""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3); t = np.asarray(t, np.float64).reshape(-1, 3)
    fx, fy, cx, cy = (F(v) for v in K)
    V = len(R)
    depth = np.full((V, rows, cols), np.nan, F); normal = np.full((V, 3, rows, cols), np.nan, F); colour = np.zeros((V, rows, cols, 3), np.uint8)
    o, h = vol.origin, vol.voxel
    with np.errstate(all="ignore"):
        for v in range(V):
            m = pose_wc(R[v], t[v])
            a = [F(F(m[9 + i] - o[i]) / h) for i in range(3)]
            for pv in range(rows):
                for pu in range(cols):
                    dx, dy = F(F(F(pu) - cx) / fx), F(F(F(pv) - cy) / fy)
                    b = [F(F(F(F(m[3 * i] * dx) + F(m[3 * i + 1] * dy)) + m[3 * i + 2]) / h) for i in range(3)]
                    pos = lambda Z: [F(a[i] + F(Z * b[i])) for i in range(3)]
                    prev, f_prev, z_prev, zs, n = None, F(0), F(0), None, 0
                    while n <= MAX_STEPS:
                        Z = F(F(z_min) + F(F(n) * F(step)))
                        if not Z <= F(z_max):
                            break
                        s = _sample_loop(vol, *pos(Z), min_weight)
                        f = _tri_loop(s[4], s[1], s[2], s[3]) if s else F(0)
                        if s and prev:
                            if f_prev > 0 and f <= 0:
                                zs = F(z_prev + F(F(f_prev / F(f_prev - f)) * F(Z - z_prev)))
                                break
                            if not f_prev > 0 and f > 0:
                                break
                        prev, f_prev, z_prev, n = s, f, Z, n + 1
                    if zs is None:
                        continue
                    depth[v, pv, pu] = zs
                    s = _sample_loop(vol, *pos(zs), min_weight)
                    if not s:
                        continue
                    corners, fx_, fy_, fz_, d = s
                    lx = [_l(d[2 * q], d[2 * q + 1], fx_) for q in range(4)]            # Lx_00 Lx_10 Lx_01 Lx_11
                    gx = _l(_l(F(d[1] - d[0]), F(d[3] - d[2]), fy_), _l(F(d[5] - d[4]), F(d[7] - d[6]), fy_), fz_)
                    gy = _l(F(lx[1] - lx[0]), F(lx[3] - lx[2]), fz_)
                    gz = F(_l(lx[2], lx[3], fy_) - _l(lx[0], lx[1], fy_))
                    L = F(np.sqrt(F(F(F(gx * gx) + F(gy * gy)) + F(gz * gz))))
                    if L > 0 and np.isfinite(L):
                        nw = [F(gx / L), F(gy / L), F(gz / L)]
                        normal[v, :, pv, pu] = [F(F(F(m[i] * nw[0]) + F(m[3 + i] * nw[1])) + F(m[6 + i] * nw[2])) for i in range(3)]
                    mean = []
                    for c in corners:
                        cn = int(vol.Cn[c[2], c[1], c[0]])
                        mean.append([F(min((2 * int(vol.rgb[ch, c[2], c[1], c[0]]) + cn) // (2 * cn), 255)) for ch in range(3)]
                                    if cn and vol.colour else None)
                    if all(x is not None for x in mean):
                        colour[v, pv, pu] = [int(min(max(np.floor(F(_tri_loop([x[ch] for x in mean], fx_, fy_, fz_) + F(0.5))), 0), 255))
                                             for ch in range(3)]
                    else:
                        near = mean[int(fx_ >= 0.5) + 2 * int(fy_ >= 0.5) + 4 * int(fz_ >= 0.5)]
                        colour[v, pv, pu] = [int(x) for x in near] if near is not None else [0, 0, 0]
    return one_nan(depth), one_nan(normal), colour


# ---- vertex normals -------------------------------------------------------------------------------------------------------------------
def active_edges(vol, min_weight):
    """step 9 in rank order -> (a, b: linear indices of the inside and the outside end, t of step 10)"""
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
        act[lin[P][valid[P] & valid[Q] & (inside[P] != inside[Q])], c - 1] = True
    e = np.nonzero(act.reshape(-1))[0]
    p, c = e // 7, e % 7 + 1
    q = p + (c & 1) + ((c >> 1) & 1) * nx + ((c >> 2) & 1) * nx * ny
    ins = inside.reshape(-1)
    a, b = np.where(ins[p], p, q), np.where(ins[p], q, p)
    D = vol.D.reshape(-1)
    with np.errstate(all="ignore"):
        tt = D[a] / (D[a] - D[b])
    return a, b, tt


def voxel_gradient(vol, min_weight):
    """step 22 for every voxel -> float32 [3, n] (x, y, z) and, for the tests, the form taken int8 [3, n]: 3 both, 2 only p + e,
    1 only p - e, 0 neither"""
    valid = vol.W >= min_weight
    D = vol.D
    g, form = [], []
    for axis in (2, 1, 0):
        n = D.shape[axis]
        shape = [1, 1, 1]; shape[axis] = n
        idx = np.arange(n).reshape(shape)
        Dp, Dm = np.roll(D, -1, axis), np.roll(D, 1, axis)
        vp, vm = np.roll(valid, -1, axis) & (idx < n - 1), np.roll(valid, 1, axis) & (idx > 0)
        with np.errstate(all="ignore"):
            ga = np.where(vp & vm, Dp - Dm, np.where(vp, F(2) * (Dp - D), np.where(vm, F(2) * (D - Dm), F(0))))
        assert ga.dtype == F
        g.append(ga.reshape(-1)); form.append((2 * vp + vm).astype(np.int8).reshape(-1))
    return np.stack(g), np.stack(form)


def vertex_normals(vol, min_weight=1):
    """steps 22 and 23 -> float32 [nv, 3] at the vertex ranks of tsdf_mirror.extract"""
    a, b, tt = active_edges(vol, min_weight)
    g, _ = voxel_gradient(vol, min_weight)
    with np.errstate(all="ignore"):
        v = [g[ax, a] + tt * (g[ax, b] - g[ax, a]) for ax in range(3)]
        L = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        ok = (L > 0) & np.isfinite(L)
        out = np.stack([np.where(ok, c / L, F(0)) for c in v], 1).astype(F)
    assert L.dtype == F
    return out


def normals_loop(vol, min_weight):
    """steps 22 and 23 as scalar loops, in the edge order of tsdf_mirror.extract_loop -> a list of [nx, ny, nz]"""
    dims = (vol.nx, vol.ny, vol.nz)
    valid = lambda p: vol.W[p[2], p[1], p[0]] >= min_weight
    Dv = lambda p: F(vol.D[p[2], p[1], p[0]])

    def grad(p, ax):
        lo, hi = list(p), list(p)
        lo[ax] -= 1; hi[ax] += 1
        has_lo, has_hi = p[ax] > 0 and valid(lo), p[ax] + 1 < dims[ax] and valid(hi)
        if has_lo and has_hi:
            return F(Dv(hi) - Dv(lo))
        if has_hi:
            return F(F(2) * F(Dv(hi) - Dv(p)))
        if has_lo:
            return F(F(2) * F(Dv(p) - Dv(lo)))
        return F(0)

    out = []
    with np.errstate(all="ignore"):
        for k in range(vol.nz):
            for j in range(vol.ny):
                for i in range(vol.nx):
                    for c in range(1, 8):
                        dx, dy, dz = offset(c)
                        p, q = (i, j, k), (i + dx, j + dy, k + dz)
                        if q[0] >= vol.nx or q[1] >= vol.ny or q[2] >= vol.nz or not (valid(p) and valid(q)):
                            continue
                        if (Dv(p) < 0) == (Dv(q) < 0):
                            continue
                        a, b = (p, q) if Dv(p) < 0 else (q, p)
                        tt = F(Dv(a) / F(Dv(a) - Dv(b)))
                        g = [F(grad(a, ax) + F(tt * F(grad(b, ax) - grad(a, ax)))) for ax in range(3)]
                        L = F(np.sqrt(F(F(F(g[0] * g[0]) + F(g[1] * g[1])) + F(g[2] * g[2]))))
                        out.append([F(x / L) for x in g] if L > 0 and np.isfinite(L) else [F(0)] * 3)
    return out
