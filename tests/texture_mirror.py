"""numpy restatement of the texturing contract (include/rgbid_texture.h), steps 1 - 8, stated twice: vectorised over
the used texels of the mesh, and as plain scalar loops over Python integers and floats (`*_loop`: steps 1 - 4, 6 and 7).  Both are
written from the contract, not from the kernels.  Step 5, the (texel, view) pair, is the recolouring contract's and is taken from
tests/recolour_mirror (view_pairs through its Recolour state): a texel's point stands where a vertex stands there.  Doubles are numpy or
Python doubles, float32 values are rounded once where the contract says (float); everything that is accumulated is an integer.

The used texels are kept triangle-major: row t * P + r of every per-texel array is texel r of triangle t, in the order of `patch_texels`."""
import numpy as np

from tests import recolour_mirror as CM

F, U8, U32, U64, I64 = np.float32, np.uint8, np.uint32, np.uint64, np.int64
MEAN, BEST = CM.MEAN, CM.BEST
NO_VIEW = CM.NO_VIEW
COUNTS = CM.COUNTS
MAX_DIM = 16384
MIN_PATCH, MAX_PATCH = 2, 30


# ---- steps 1 - 3 ---------------------------------------------------------------------------------------------------------------------------
def layout(n_t, n, tiles_x):
    """step 1 -> dict(T, W, H, tiles, tile_rows, tiles_x, texels_per_triangle)"""
    assert 0 <= n_t <= 2 ** 31 - 1 and MIN_PATCH <= n <= MAX_PATCH and tiles_x >= 1
    T, tiles = n + 2, (n_t + 1) // 2
    tile_rows = max(1, -(-tiles // tiles_x))
    assert tiles_x * T <= MAX_DIM and tile_rows * T <= MAX_DIM
    return dict(T=T, W=tiles_x * T, H=tile_rows * T, tiles=tiles, tile_rows=tile_rows, tiles_x=tiles_x, texels_per_triangle=n * (n + 1) // 2 + (n - 1))


def patch_texels(n):
    """steps 2 and 3 of the lower half -> (i, j, wa, wb, wc) int64 [P]: the tile-local texels row by row, and their weights over n - 1"""
    j, i = np.mgrid[0:n + 2, 0:n + 2]
    use = (i + j <= n - 1) | ((i + j == n) & (i >= 1) & (i <= n - 1))
    i, j = i[use].astype(I64), j[use].astype(I64)
    return i, j, (n - 1) - i - j, i, j


def atlas_pixels(n_t, n, tiles_x):
    """-> (col, row) int64 [n_t, P]: where each used texel lies in the atlas"""
    i, j, _, _, _ = patch_texels(n)
    T = n + 2
    t = np.arange(n_t, dtype=I64)[:, None]
    up = (t & 1) == 1
    li, lj = np.where(up, T - 1 - i[None], i[None]), np.where(up, T - 1 - j[None], j[None])
    tile = t >> 1
    return (tile % tiles_x) * T + li, (tile // tiles_x) * T + lj


# ---- step 4 ------------------------------------------------------------------------------------------------------------------------------
def mix(values, tri, n):
    """step 4: float32 per-vertex rows [n_v, 3] -> float32 [n_t * P, 3] at the used texels"""
    _, _, wa, wb, wc = patch_texels(n)
    A, B, Cc = (np.ascontiguousarray(values, F)[tri[:, k]].astype(np.float64)[:, None, :] for k in range(3))     # [n_t, 1, 3]
    wa, wb, wc = (w.astype(np.float64)[None, :, None] for w in (wa, wb, wc))
    with np.errstate(all="ignore"):
        p = ((wa * A + wb * B) + wc * Cc) / np.float64(n - 1)
        return p.astype(F).reshape(-1, 3)


def _tri(triangles, n_v):
    tri = np.ascontiguousarray(np.asarray(triangles).reshape(-1, 3)).astype(I64) & 0xFFFFFFFF
    if len(tri) and (n_v == 0 or tri.max() >= n_v):
        raise ValueError("a triangle names a vertex that does not exist")
    return tri


# ---- steps 6 and 7 -------------------------------------------------------------------------------------------------------------------------
def fallback(colours_in, tri, n):
    """step 6's colour of a texel no view took -> uint8 [n_t * P, 3]"""
    _, _, wa, wb, wc = patch_texels(n)
    ca, cb, cc = (np.ascontiguousarray(colours_in, U8).reshape(-1, 3)[tri[:, k]].astype(I64)[:, None, :] for k in range(3))
    q = (wa[None, :, None] * ca + wb[None, :, None] * cb) + wc[None, :, None] * cc
    D = n - 1
    return np.clip((2 * q + D) // (2 * D), 0, 255).astype(U8).reshape(-1, 3)      # numpy's // floors


def uv_of(n_t, n, tiles_x):
    """step 7 -> float32 [n_t, 3, 2]"""
    L = layout(n_t, n, tiles_x)
    T, W, H = L["T"], L["W"], L["H"]
    t = np.arange(n_t, dtype=I64)[:, None]
    ci, cj = np.array([[0, n - 1, 0]], I64), np.array([[0, 0, n - 1]], I64)
    up = (t & 1) == 1
    col = ((t >> 1) % tiles_x) * T + np.where(up, T - 1 - ci, ci)
    row = ((t >> 1) // tiles_x) * T + np.where(up, T - 1 - cj, cj)
    u = ((2 * col + 1).astype(np.float64) / np.float64(2 * W)).astype(F)
    v = ((2 * (H - 1 - row) + 1).astype(np.float64) / np.float64(2 * H)).astype(F)
    return np.stack([u, v], -1).astype(F).reshape(n_t, 3, 2)


class Texture:
    """the handle's state and calls: begin is the constructor"""

    def __init__(self, n_t, n, tiles_x, mode=MEAN):
        self.L = layout(n_t, n, tiles_x)
        self.n_t, self.n, self.tiles_x = int(n_t), int(n), int(tiles_x)
        self.P = self.L["texels_per_triangle"]
        self.h = CM.Recolour(self.n_t * self.P, mode)          # steps 5's sums, one entry per used texel

    @property
    def mode(self):
        return self.h.mode

    @property
    def counts(self):
        return self.h.counts

    def add(self, vertices, triangles, R, t, K, rows, cols, colours, surface=None, depthinv=None, normals=None, **params):
        pos = np.ascontiguousarray(vertices, F).reshape(-1, 3)
        tri = _tri(triangles, len(pos))
        assert len(tri) == self.n_t
        p = mix(pos, tri, self.n)
        nrm = None if normals is None else mix(np.ascontiguousarray(normals, F).reshape(-1, 3), tri, self.n)
        self.h.add(p, R, t, K, rows, cols, colours, surface, depthinv, nrm, **params)

    def state_bytes(self):
        return self.h.state_bytes()

    def finish(self, triangles=None, colours_in=None):
        """step 6 -> dict(atlas uint8 [H, W, 3], views_used uint32 [H, W], and for BEST best_view uint32 [H, W])"""
        H, W = self.L["H"], self.L["W"]
        res = self.h.finish()                                  # the used texels; those no view took are 0 0 0 there
        col = res["colours"]
        if colours_in is not None and self.n_t:
            cin = np.ascontiguousarray(colours_in, U8).reshape(-1, 3)
            fb = fallback(cin, _tri(triangles, len(cin)), self.n)
            unseen = res["views_used"] == 0
            col[unseen] = fb[unseen]
        cx, ry = atlas_pixels(self.n_t, self.n, self.tiles_x)
        cx, ry = cx.reshape(-1), ry.reshape(-1)
        out = dict(atlas=np.zeros((H, W, 3), U8), views_used=np.zeros((H, W), U32))
        out["atlas"][ry, cx] = col
        out["views_used"][ry, cx] = res["views_used"]
        if self.mode == BEST:
            out["best_view"] = np.full((H, W), NO_VIEW, U32)
            out["best_view"][ry, cx] = res["best_view"]
        return out

    def uv(self):
        return uv_of(self.n_t, self.n, self.tiles_x)


def texture_numpy(vertices, triangles, R, t, K, rows, cols, colours, patch, tiles_x, mode=MEAN, colours_in=None, split=None, **kw):
    """begin, add (the views in calls of `split` views each: None = one call), finish, uv -> finish's dict with uv, counts int64 [V, 6]
    and the state's bytes"""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3); t = np.asarray(t, np.float64).reshape(-1, 3)
    V = len(R)
    h = Texture(len(np.asarray(triangles).reshape(-1, 3)), patch, tiles_x, mode)
    step = max(V, 1) if split is None else split
    part = lambda x, a: None if x is None else x[a:a + step]
    for a in range(0, V, step):
        h.add(vertices, triangles, R[a:a + step], t[a:a + step], K, rows, cols, colours[a:a + step], part(kw.get("surface"), a), part(kw.get("depthinv"), a),
              **{k: v for k, v in kw.items() if k not in ("surface", "depthinv")})
    out = h.finish(triangles, colours_in)
    out["uv"] = h.uv()
    out["counts"] = h.counts
    out["state"] = h.state_bytes()
    return out


# ---- the scalar restatement: steps 1 - 4, 6 and 7 one texel at a time ------------------------------------------------------------------------
def texels_loop(n):
    """steps 2 and 3 of the lower half -> [(i, j, wa, wb, wc)] row by row"""
    out = []
    for j in range(n + 2):
        for i in range(n + 2):
            if i + j <= n - 1 or (i + j == n and 1 <= i <= n - 1):
                out.append((i, j, (n - 1) - i - j, i, j))
    return out


def place_loop(t, i, j, n, tiles_x):
    """steps 1 and 2: lower-half texel (i, j) of triangle t -> (col, row) in the atlas"""
    T = n + 2
    if t & 1:
        i, j = T - 1 - i, T - 1 - j
    tile = t >> 1
    return (tile % tiles_x) * T + i, (tile // tiles_x) * T + j


def mix_loop(wa, wb, wc, n, a, b, c):
    """step 4 for one component: float32 corners -> float32"""
    with np.errstate(all="ignore"):
        s = (np.float64(wa) * np.float64(a) + np.float64(wb) * np.float64(b)) + np.float64(wc) * np.float64(c)
        return F(s / np.float64(n - 1))


def points_loop(values, triangles, n):
    """step 4 -> float32 [n_t * P, 3]"""
    values = np.ascontiguousarray(values, F).reshape(-1, 3)
    out = []
    for a, b, c in np.asarray(triangles).reshape(-1, 3).tolist():
        for _, _, wa, wb, wc in texels_loop(n):
            out.append([mix_loop(wa, wb, wc, n, values[a][k], values[b][k], values[c][k]) for k in range(3)])
    return np.array(out, F).reshape(-1, 3)


def fallback_loop(wa, wb, wc, n, ca, cb, cc):
    """step 6's byte of a texel no view took, in Python integers"""
    q = (wa * int(ca) + wb * int(cb)) + wc * int(cc)
    return min(255, max(0, (2 * q + (n - 1)) // (2 * (n - 1))))


def finish_loop(state, used, mode, triangles, n, tiles_x, colours_in=None):
    """step 6 from the sums of the used texels (state uint64 [4, n_t * P], used uint32 [n_t * P]) -> dict(atlas, views_used, best_view)"""
    tri = np.asarray(triangles).reshape(-1, 3).tolist()
    L = layout(len(tri), n, tiles_x)
    out = dict(atlas=np.zeros((L["H"], L["W"], 3), U8), views_used=np.zeros((L["H"], L["W"]), U32), best_view=np.full((L["H"], L["W"]), 0xFFFFFFFF, U32))
    tex = texels_loop(n)
    for t, (a, b, c) in enumerate(tri):
        for r, (i, j, wa, wb, wc) in enumerate(tex):
            col, row = place_loop(t, i, j, n, tiles_x)
            e = t * len(tex) + r
            S, u = [int(x) for x in state[:, e]], int(used[e])
            out["views_used"][row, col] = u
            if u and mode == MEAN:
                out["atlas"][row, col] = [(2 * S[k] + 65536 * S[3]) // (2 * 65536 * S[3]) for k in range(3)]
            elif u:
                out["atlas"][row, col] = [(S[k] + 32768) >> 16 for k in range(3)]
                out["best_view"][row, col] = 0xFFFFFFFF - (S[3] & 0xFFFFFFFF)
            elif colours_in is not None:
                out["atlas"][row, col] = [fallback_loop(wa, wb, wc, n, colours_in[a][k], colours_in[b][k], colours_in[c][k]) for k in range(3)]
    if mode != BEST:
        del out["best_view"]
    return out


def uv_loop(n_t, n, tiles_x):
    """step 7 -> float32 [n_t, 3, 2]"""
    L = layout(n_t, n, tiles_x)
    out = np.zeros((n_t, 3, 2), F)
    for t in range(n_t):
        for c, (i, j) in enumerate(((0, 0), (n - 1, 0), (0, n - 1))):
            col, row = place_loop(t, i, j, n, tiles_x)
            out[t, c] = F((2 * col + 1) / (2 * L["W"])), F((2 * (L["H"] - 1 - row) + 1) / (2 * L["H"]))
    return out


def texture_loop(vertices, triangles, R, t, K, rows, cols, colours, patch, tiles_x, mode=MEAN, colours_in=None, normals=None, **kw):
    """the contract with steps 1 - 4, 6 and 7 as loops -> texture_numpy's dict without the state"""
    tri = np.asarray(triangles).reshape(-1, 3)
    h = CM.Recolour(len(tri) * len(texels_loop(patch)), mode)
    h.add(points_loop(vertices, tri, patch), R, t, K, rows, cols, colours, kw.pop("surface", None), kw.pop("depthinv", None),
          None if normals is None else points_loop(normals, tri, patch), **kw)
    out = finish_loop(h.a, h.used, h.mode, tri, patch, tiles_x, colours_in)
    out["uv"] = uv_loop(len(tri), patch, tiles_x)
    out["counts"] = h.counts
    return out


# ---- a bilinear look-up, as a viewer makes it ------------------------------------------------------------------------------------------------
def lookup(atlas, u, v):
    """the atlas (any dtype [H, W, C]) filtered bilinearly at uv (origin bottom-left, texel centres at half-integers, clamped at the border)
    -> (float64 [C], [(col, row, weight)] of the four taps)"""
    H, W = atlas.shape[:2]
    x, y = u * W - 0.5, (1.0 - v) * H - 0.5
    x0, y0 = int(np.floor(x)), int(np.floor(y))
    ax, ay = x - x0, y - y0
    taps = [(x0, y0, (1 - ax) * (1 - ay)), (x0 + 1, y0, ax * (1 - ay)), (x0, y0 + 1, (1 - ax) * ay), (x0 + 1, y0 + 1, ax * ay)]
    taps = [(min(max(c, 0), W - 1), min(max(r, 0), H - 1), w) for c, r, w in taps]
    return sum(w * atlas[r, c].astype(np.float64) for c, r, w in taps), taps
