"""Numpy restatement of the radius outlier contract (include/rgbid_outlier.h) that the GPU tests compare the
kernels against: the brute-force definition over every pair in float32, in the contract's operation order, and for large clouds an
independent float64 grid of cells >= 2 r that only selects the candidates the same float32 distance test then judges."""
import numpy as np

from rgbid import cloud as CL
from rgbid import outlier as OL


def _fields(points):
    return np.ascontiguousarray(points).view(CL.POINT_DTYPE).reshape(-1) if not (isinstance(points, np.ndarray) and points.dtype.names) else points


def _finite(p):
    return np.isfinite(p["x"]) & np.isfinite(p["y"]) & np.isfinite(p["z"])


def _d2_le(xi, yi, zi, xj, yj, zj, r2):
    """d2 = (dx dx + dy dy) + dz dz <= r2 with d = p_j - p_i: every operation one float32 numpy call, so no contraction"""
    with np.errstate(all="ignore"):
        dx, dy, dz = xj - xi, yj - yi, zj - zi
        assert dx.dtype == np.float32
        return (dx * dx + dy * dy) + dz * dz <= r2


def radius_counts_bruteforce(points, r, cap, block=512):
    """count[i] = min(#{j != i taking part : d2(i, j) <= r2}, cap) over every pair, blocked O(n^2); 0 for records that take no part"""
    p = _fields(points)
    r = np.float32(r)
    r2 = r * r
    fin = _finite(p)
    src = np.nonzero(fin)[0]
    x, y, z = (np.ascontiguousarray(p[c][src]) for c in "xyz")
    cnt = np.zeros(src.size, np.int64)
    for b in range(0, src.size, block):
        s = slice(b, b + block)
        hit = _d2_le(x[s, None], y[s, None], z[s, None], x[None, :], y[None, :], z[None, :], r2)
        cnt[s] = hit.sum(1) - 1                                  # the point itself: d2 = 0 <= r2
    out = np.zeros(len(p), np.int64)
    out[src] = np.minimum(cnt, int(cap))
    return out


def radius_counts_grid(points, r, cap, chunk=1 << 22):
    """the same counts through a float64 grid with cells of 2.5 r: two points the float32 test accepts are at most r (1 + 2^-21) apart
    on every axis, less than half a cell, so they lie in the same or in adjacent cells whatever the float64 rounding does"""
    p = _fields(points)
    r = np.float32(r)
    r2 = r * r
    fin = _finite(p)
    src = np.nonzero(fin)[0]
    out = np.zeros(len(p), np.int64)
    if src.size == 0:
        return out
    xyz = [np.ascontiguousarray(p[c][src]) for c in "xyz"]
    cell = 2.5 * float(r)
    ijk = np.stack([np.floor(c.astype(np.float64) / cell).astype(np.int64) for c in xyz], 1)
    ijk -= ijk.min(0)
    dims = ijk.max(0) + 3                                        # one empty cell on every side: neighbour keys never wrap
    assert float(dims[0]) * float(dims[1]) * float(dims[2]) < 2.0 ** 62
    key = ((ijk[:, 2] + 1) * dims[1] + (ijk[:, 1] + 1)) * dims[0] + (ijk[:, 0] + 1)
    order = np.argsort(key, kind="stable")
    sk = key[order]
    sx, sy, sz = (c[order] for c in xyz)
    ukeys, starts, sizes = np.unique(sk, return_index=True, return_counts=True)
    cnt = np.zeros(src.size, np.int64)                           # in sorted order
    for dk in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                nk = sk + ((dk * dims[1] + dj) * dims[0] + di)
                c = np.searchsorted(ukeys, nk)
                ok = (c < len(ukeys)) & (ukeys[np.minimum(c, len(ukeys) - 1)] == nk)
                who = np.nonzero(ok)[0]
                beg, num = starts[c[who]], sizes[c[who]]
                tot = np.cumsum(num)
                lo = 0
                while lo < len(who):                             # chunks of about `chunk` pairs
                    base = tot[lo - 1] if lo else 0
                    hi = max(int(np.searchsorted(tot, base + chunk, side="right")), lo + 1)
                    n_ = num[lo:hi]
                    i = np.repeat(who[lo:hi], n_)
                    off = np.arange(int(n_.sum())) - np.repeat(tot[lo:hi] - n_ - base, n_)
                    j = np.repeat(beg[lo:hi], n_) + off
                    hit = _d2_le(sx[i], sy[i], sz[i], sx[j], sy[j], sz[j], r2) & (i != j)
                    cnt += np.bincount(i[hit], minlength=src.size)
                    lo = hi
    back = np.empty(src.size, np.int64)
    back[order] = cnt
    out[src] = np.minimum(back, int(cap))
    return out


def radius_filter_numpy(points, r, min_neighbours, cap=None, counts=None, brute_below=20_000):
    """-> (counts int64 [n], mask bool [n], kept records): the contract on rgbid_cloud_point records (structured POINT_DTYPE or [M, 32]
    uint8); brute force up to brute_below records, the grid above"""
    OL.radius32(r)
    m, c = OL.neighbour_args(min_neighbours, cap)
    p = _fields(points)
    if counts is None:
        counts = radius_counts_bruteforce(p, r, c) if len(p) <= brute_below else radius_counts_grid(p, r, c)
    mask = _finite(p) & (counts >= m)
    return counts, mask, p[mask]
