"""numpy restatement of the recolouring contract (include/rgbid_recolour.h), steps 1 - 8, vectorised over the
vertices of one view at a time, with uint64 sums.  Written from the contract, not from the kernel.  Step 3 is the rasteriser's
(tests/raster_mirror.project); float32 operations are numpy float32 arrays (one rounding per operation), doubles are numpy doubles,
everything that is accumulated is an integer."""
import numpy as np

from tests import raster_mirror as XM
from tests.render_mirror import pose_cw

F, U8, U32, U64, I64 = np.float32, np.uint8, np.uint32, np.uint64, np.int64
MEAN, BEST = 0, 1
MODES = {"mean": MEAN, "best": BEST}
MAX_VIEWS = 65535
UNIT = 1024
NO_VIEW = U32(0xFFFFFFFF)
COUNTS = ("gated", "outside", "hidden", "unmeasured", "averted", "taken")
GATED, OUTSIDE, HIDDEN, UNMEASURED, AVERTED, TAKEN = range(6)


def footprint(xs, ys, rows, cols):
    """step 4's footprint of snapped positions inside the image -> (flat texel indices [4, n] in the order 00 10 01 11, ax, ay)"""
    x0, y0 = xs >> 8, ys >> 8
    x1, y1 = np.minimum(x0 + 1, cols - 1), np.minimum(y0 + 1, rows - 1)
    return np.stack([y0 * cols + x0, y0 * cols + x1, y1 * cols + x0, y1 * cols + x1]), xs & 255, ys & 255


def cosine(nrm, m, X, Y, Z, two_sided):
    """step 4's facing test -> (facing bool: the normal has a finite, non-zero squared length; cos float64)"""
    n0, n1, n2 = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    with np.errstate(all="ignore"):
        q = (n0 * n0 + n1 * n1) + n2 * n2
        c = [((m[3 * k] * n0 + m[3 * k + 1] * n1) + m[3 * k + 2] * n2) for k in range(3)]
        assert q.dtype == F and c[0].dtype == F
        c0, c1, c2 = (x.astype(np.float64) for x in c)
        Xd, Yd, Zd = X.astype(np.float64), Y.astype(np.float64), Z.astype(np.float64)
        dot = -((c0 * Xd + c1 * Yd) + c2 * Zd)
        g = (c0 * c0 + c1 * c1) + c2 * c2
        r = (Xd * Xd + Yd * Yd) + Zd * Zd
        cos = dot / np.sqrt(g * r)
    return np.isfinite(q) & (q != 0), np.abs(cos) if two_sided else cos


def view_pairs(pos, nrm, m, K, rows, cols, colour, surface, measured, z_min, z_max, tol_surface, tol_measured, min_cos, two_sided):
    """steps 3 - 5 of one view -> (cls int [n_v], taken: indices of the TAKEN vertices, w uint64 and s uint64 [., 3] of those)"""
    xs, ys, Z, ok = XM.project(pos, m, K, z_min, z_max)
    cls = np.full(len(pos), GATED)
    inside = ok & (xs >= 0) & (xs <= 256 * (cols - 1)) & (ys >= 0) & (ys <= 256 * (rows - 1))
    cls[ok & ~inside] = OUTSIDE
    idx = np.flatnonzero(inside)
    tex, ax, ay = footprint(xs[idx], ys[idx], rows, cols)
    Zi = Z[idx]
    live = np.ones(len(idx), bool)
    with np.errstate(all="ignore"):
        if surface is not None:
            d = np.ascontiguousarray(surface, F).reshape(-1)[tex]
            bad = (~np.isfinite(d) | (np.abs(Zi[None] - d) > F(tol_surface))).any(0)
            cls[idx[bad]] = HIDDEN
            live &= ~bad
        if measured is not None:
            iD = np.ascontiguousarray(measured, F).reshape(-1)[tex]
            z = F(1) / iD
            assert z.dtype == F
            bad = live & (~np.isfinite(iD) | ~(iD > 0) | ~np.isfinite(z) | (np.abs(Zi[None] - z) > F(tol_measured))).any(0)
            cls[idx[bad]] = UNMEASURED
            live &= ~bad
        w = np.full(len(idx), UNIT, U64)
        if nrm is not None:
            p = pos[idx]
            X = ((m[0] * p[:, 0] + m[1] * p[:, 1]) + m[2] * p[:, 2]) + m[9]
            Y = ((m[3] * p[:, 0] + m[4] * p[:, 1]) + m[5] * p[:, 2]) + m[10]
            facing, cos = cosine(nrm[idx], m, X, Y, Zi, two_sided)
            good = (cos > 0) & (cos >= np.float64(F(min_cos)))
            bad = live & facing & ~good
            cls[idx[bad]] = AVERTED
            live &= ~bad
            use = live & facing
            w[use] = np.maximum(1, np.floor(cos[use] * 1024.0 + 0.5)).astype(U64)
    cls[idx[live]] = TAKEN
    tex, ax, ay = tex[:, live].astype(I64), ax[live].astype(U64), ay[live].astype(U64)
    col = np.ascontiguousarray(colour, U8).reshape(-1, 3).astype(U64)
    one = U64(256)
    s = ((one - ax) * (one - ay))[:, None] * col[tex[0]] + (ax * (one - ay))[:, None] * col[tex[1]] + ((one - ax) * ay)[:, None] * col[tex[2]] \
        + (ax * ay)[:, None] * col[tex[3]]
    assert s.dtype == U64 and (not s.size or int(s.max()) <= 255 * 65536)
    return cls, idx[live], w[live], s


class Recolour:
    """the handle's state and calls: begin is the constructor"""

    def __init__(self, n_vertices, mode=MEAN):
        mode = MODES.get(mode, mode)
        assert mode in (MEAN, BEST) and n_vertices >= 0
        self.n, self.mode, self.views = int(n_vertices), mode, 0
        self.a = np.zeros((4, self.n), U64)            # MEAN: S_0 S_1 S_2 W; BEST: s_0 s_1 s_2 key
        self.used = np.zeros(self.n, U32)
        self.counts = np.zeros((0, 6), I64)

    def add(self, vertices, R, t, K, rows, cols, colours, surface=None, depthinv=None, normals=None, z_min=0.05, z_max=20.0,
            surface_tolerance=0.02, measured_tolerance=0.02, min_cos=0.2, two_sided=False):
        pos = np.ascontiguousarray(vertices, F).reshape(-1, 3)
        nrm = None if normals is None else np.ascontiguousarray(normals, F).reshape(-1, 3)
        R = np.asarray(R, np.float64).reshape(-1, 3, 3); t = np.asarray(t, np.float64).reshape(-1, 3)
        V = len(R)
        assert len(pos) == self.n and (nrm is None or len(nrm) == self.n) and V >= 1 and self.views + V <= MAX_VIEWS and len(colours) == V
        for v in range(V):
            cls, taken, w, s = view_pairs(pos, nrm, pose_cw(R[v], t[v]), K, rows, cols, colours[v], None if surface is None else surface[v],
                                          None if depthinv is None else depthinv[v], z_min, z_max, surface_tolerance, measured_tolerance, min_cos,
                                          two_sided)
            self.counts = np.concatenate([self.counts, [[int((cls == k).sum()) for k in range(6)]]])
            self.used[taken] += U32(1)
            if self.mode == MEAN:
                self.a[:3, taken] += (w[:, None] * s).T
                self.a[3, taken] += w
            else:
                key = (w << U64(32)) | U64(0xFFFFFFFF - self.views)
                wins = key > self.a[3, taken]
                self.a[:3, taken[wins]] = s[wins].T
                self.a[3, taken[wins]] = key[wins]
            self.views += 1

    def state_bytes(self):
        return self.a.tobytes() + self.used.tobytes()

    def finish(self, colours_in=None):
        """step 7 -> dict(colours uint8 [n, 3], views_used uint32 [n], and for BEST best_view uint32 [n])"""
        seen = self.used > 0
        out = np.zeros((self.n, 3), U8) if colours_in is None else np.array(colours_in, U8).reshape(-1, 3).copy()
        if self.mode == MEAN:
            D = U64(65536) * self.a[3, seen]
            out[seen] = ((U64(2) * self.a[:3, seen] + D) // (U64(2) * D)).T.astype(U8)
        else:
            out[seen] = ((self.a[:3, seen] + U64(32768)) >> U64(16)).T.astype(U8)
        res = dict(colours=out, views_used=self.used.copy())
        if self.mode == BEST:
            res["best_view"] = np.where(seen, U64(0xFFFFFFFF) - (self.a[3] & U64(0xFFFFFFFF)), U64(NO_VIEW)).astype(U32)
        return res


def recolour_numpy(vertices, R, t, K, rows, cols, colours, mode=MEAN, colours_in=None, split=None, **kw):
    """begin, add (the views in calls of `split` views each: None = one call), finish -> finish's dict with counts int64 [V, 6] and the
    state's bytes"""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3); t = np.asarray(t, np.float64).reshape(-1, 3)
    V = len(R)
    h = Recolour(len(np.asarray(vertices).reshape(-1, 3)), mode)
    step = V if split is None else split
    part = lambda x, a: None if x is None else x[a:a + step]
    for a in range(0, V, step):
        h.add(vertices, R[a:a + step], t[a:a + step], K, rows, cols, colours[a:a + step], part(kw.get("surface"), a), part(kw.get("depthinv"), a),
              **{k: v for k, v in kw.items() if k not in ("surface", "depthinv")})
    out = h.finish(colours_in)
    out["counts"] = h.counts
    out["state"] = h.state_bytes()
    return out
