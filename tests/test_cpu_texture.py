"""CPU checks of the texturing stage (include/rgbid_texture.h, rgbid.texture): the layout's claims re-derived for every patch size; the
layout against hand values and against the library's host function; the numpy restatement the GPU tests compare the kernels against
(tests/texture_mirror.py) against its scalar restatement; a case written out by hand; the fallback's rounding and clamps; non-finite
corners; shared edges; the texture coordinates; a linear ramp looked up bilinearly; the Python argument checks; the header as C99; the
library's exports and NULL-handle refusals; the OBJ files; the command line's option errors."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from rgbid import _lib
from rgbid import recolour as RC
from rgbid import texture as TX
from tests import recolour_mirror as CM
from tests import texture_mirror as TM
from tests.test_cpu_recolour import OPTIONAL, PARAMS, UNIT, random_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
F, U8, U32 = np.float32, np.uint8, np.uint32
EYE, ZERO = np.eye(3)[None], np.zeros((1, 3))
PATCHES = range(2, 31)


def mesh_case(vertices, triangles, colours, K=UNIT, R=EYE, t=ZERO, normals=None, surface=None, depthinv=None, patch=2, tiles_x=1, **params):
    """tests.test_cpu_recolour.case with triangles, a patch size and tiles_x"""
    col = np.ascontiguousarray(colours, U8)
    V, rows, cols = col.shape[:3]
    R, t = np.asarray(R, np.float64).reshape(-1, 3, 3), np.asarray(t, np.float64).reshape(-1, 3)
    if len(R) == 1 and V > 1:
        R, t = np.repeat(R, V, 0), np.repeat(t, V, 0)
    plane = lambda x: None if x is None else np.ascontiguousarray(np.broadcast_to(np.asarray(x, F), (V, rows, cols)))
    return dict(vertices=np.array(vertices, F).reshape(-1, 3), triangles=np.array(triangles, U32).reshape(-1, 3),
                normals=None if normals is None else np.array(normals, F).reshape(-1, 3), R=R, t=t, K=K, rows=rows, cols=cols, colours=col,
                surface=plane(surface), depthinv=plane(depthinv), patch=patch, tiles_x=tiles_x, params=dict(PARAMS, **params))


def mirror(c, mode="mean", split=None, colours_in=None, drop=()):
    """the mirror's result of a case, without the optional inputs named in `drop`"""
    opt = {k: None if k in drop else c[k] for k in OPTIONAL}
    return TM.texture_numpy(c["vertices"], c["triangles"], c["R"], c["t"], c["K"], c["rows"], c["cols"], c["colours"], c["patch"], c["tiles_x"], mode,
                            colours_in, split, **opt, **c["params"])


def loops(c, mode="mean", colours_in=None, drop=()):
    opt = {k: None if k in drop else c[k] for k in OPTIONAL}
    return TM.texture_loop(c["vertices"], c["triangles"], c["R"], c["t"], c["K"], c["rows"], c["cols"], c["colours"], c["patch"], c["tiles_x"], mode,
                           colours_in, **opt, **c["params"])


def same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in b)


def random_mesh_case(n_v, n_t, V, patch, tiles_x, rows=12, cols=16, seed=0):
    """random_case's vertices, normals, views and planes under n_t random triangles"""
    c = random_case(n_v, V, rows, cols, seed=seed)
    rng = np.random.default_rng(1000 + seed)
    tri = rng.integers(0, n_v, (n_t, 3)).astype(U32)
    return dict(c, triangles=tri, patch=patch, tiles_x=tiles_x)


# ---- the layout ------------------------------------------------------------------------------------------------------------------------
def half_sets(n):
    """the tile-local texel sets of the two halves, from step 2's wording"""
    T = n + 2
    lower = {(i, j) for j in range(T) for i in range(T) if i + j <= n - 1 or (i + j == n and 1 <= i <= n - 1)}
    return lower, {(T - 1 - i, T - 1 - j) for i, j in lower}


@pytest.mark.parametrize("n", PATCHES)
def test_layout_claims(n):
    """the sets are disjoint, lie in the tile and hold P texels; a bilinear look-up at any point of a half's uv triangle (corners on the
    texel centres (0, 0), (n - 1, 0), (0, n - 1), mirrored for the upper half) has non-zero weight only on texels of that half's set"""
    T, P = n + 2, n * (n + 1) // 2 + (n - 1)
    lower, upper = half_sets(n)
    assert not lower & upper and len(lower) == len(upper) == P
    assert all(0 <= i < T and 0 <= j < T for i, j in lower | upper)
    i, j, wa, wb, wc = TM.patch_texels(n)
    assert set(zip(i.tolist(), j.tolist())) == lower and [tuple(x) for x in np.stack([i, j, wa, wb, wc], 1).tolist()] == TM.texels_loop(n)
    assert (wa + wb + wc == n - 1).all() and wa.min() == -1 and ((wa == -1) == (i + j == n)).all()
    rng = np.random.default_rng(n)
    b = rng.dirichlet((1, 1, 1), 2000)
    b = np.concatenate([b, np.eye(3), [[0.5, 0.5, 0], [0, 0.5, 0.5], [0.5, 0, 0.5]]])        # the corners, the edges' middles, points on the edges
    edge = rng.random(300)
    b = np.concatenate([b, np.stack([edge, 1 - edge, 0 * edge], 1), np.stack([0 * edge, edge, 1 - edge], 1), np.stack([edge, 0 * edge, 1 - edge], 1)])
    x, y = b[:, 1] * (n - 1), b[:, 2] * (n - 1)                 # the point in texel-centre coordinates of the lower half
    for name, own, px, py in (("lower", lower, x, y), ("upper", upper, T - 1 - x, T - 1 - y)):
        x0, y0 = np.floor(px).astype(int), np.floor(py).astype(int)
        ax, ay = px - x0, py - y0
        for dx, dy, w in ((0, 0, (1 - ax) * (1 - ay)), (1, 0, ax * (1 - ay)), (0, 1, (1 - ax) * ay), (1, 1, ax * ay)):
            hit = w > 0
            taps = set(zip((x0 + dx)[hit].tolist(), (y0 + dy)[hit].tolist()))
            assert taps <= own, (name, sorted(taps - own)[:4])


def test_layout_hand_values():
    """patch 2: T = 4, P = 4"""
    want = {(0, 1): (4, 4, 0, 1), (1, 1): (4, 4, 1, 1), (2, 1): (4, 4, 1, 1), (3, 1): (4, 8, 2, 2),
            (0, 2): (8, 4, 0, 1), (1, 2): (8, 4, 1, 1), (2, 2): (8, 4, 1, 1), (3, 2): (8, 4, 2, 1)}
    for (n_t, tx), (W, H, tiles, tile_rows) in want.items():
        for lay in (TX.layout(n_t, 2, tx), TM.layout(n_t, 2, tx)):
            assert (lay["T"], lay["W"], lay["H"], lay["tiles"], lay["tile_rows"], lay["texels_per_triangle"]) == (4, W, H, tiles, tile_rows, 4)
        assert TX.layout(n_t, 2, tx)["slots"] == 16 * tiles
    assert TX.layout(5, 6)["tiles_x"] == 2 and TX.layout(0, 6)["tiles_x"] == 1 and TX.layout(2, 6)["tiles_x"] == 1 and TX.layout(19, 6)["tiles_x"] == 4
    assert TX.layout(18, 6)["tiles_x"] == 3 and TX.layout(5, 6) == dict(T=8, W=16, H=16, tiles=3, tile_rows=2, tiles_x=2, texels_per_triangle=26, slots=192)
    assert TX.layout(1, 30)["texels_per_triangle"] == 494 and TX.layout(1, 14)["T"] == 16


def test_host_layout_against_python():
    _lib.build()
    rng = np.random.default_rng(4)
    cases = [(0, 2, 1), (1, 2, 1), (2, 2, 2), (3, 2, 1), (3, 2, 2), (129, 14, 3), (1 << 25, 2, 4096), (1024, 30, 1), (7, 30, 512)]
    cases += [(int(rng.integers(0, 5000)), int(rng.integers(2, 31)), int(rng.integers(1, 60))) for _ in range(50)]
    for n_t, n, tx in cases:
        want = TX.layout(n_t, n, tx)
        assert TX.host_layout(n_t, n, tx) == {k: want[k] for k in ("T", "W", "H", "tiles", "tile_rows", "texels_per_triangle")}, (n_t, n, tx)
    # each refusal: the last legal value is taken, the first beyond it is not, by the library and by the Python layer alike
    for good, bad in (((10, 2, 1), (10, 1, 1)), ((10, 30, 1), (10, 31, 1)), ((10, 6, 1), (10, 6, 0)), ((7, 30, 512), (7, 30, 513)),
                      ((1024, 30, 1), (1025, 30, 1)), ((1 << 25, 2, 4096), ((1 << 25) + 1, 2, 4096)), ((10, 6, 1), (10, 6, -1)),
                      ((10, 6, 1), ((1 << 31) - 1, 2, 4096)), ((10, 6, 1), (1 << 31, 2, 4096)), ((10, 6, 1), (10, 0, 1))):
        assert TX.host_layout(*good) is not None and TX.layout(*good)
        assert TX.host_layout(*bad) is None, bad
        with pytest.raises(ValueError):
            TX.layout(*bad)
    L = _lib.bind(TX.SIGNATURES)
    assert L.rgbid_texture_layout(10, 6, 1, None) == -1
    assert ctypes.sizeof(TX.Layout) == 32


# ---- the restatements --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mean", "best"])
@pytest.mark.parametrize("drop", [(), ("normals",), ("surface",), ("depthinv",), ("surface", "depthinv"), OPTIONAL])
@pytest.mark.parametrize("n", [2, 3, 6])
def test_mirror_against_the_scalar_restatement(mode, drop, n):
    seen = np.zeros(6, np.int64)
    for seed in range(3):
        n_t = (40, 7, 1)[seed]
        c = random_mesh_case(30, n_t, 3, n, (1, 3, 2)[seed], seed=seed + 10 * len(drop) + n)
        cin = np.random.default_rng(seed).integers(0, 256, (30, 3)).astype(U8) if seed != 1 else None
        got, want = mirror(c, mode, colours_in=cin, drop=drop), loops(c, mode, cin, drop)
        assert same(got, want), (seed, got["counts"], want["counts"])
        assert (got["counts"].sum(1) == n_t * TX.layout(n_t, n, 1)["texels_per_triangle"]).all()
        assert got["atlas"].shape == (TX.layout(n_t, n, c["tiles_x"])["H"], TX.layout(n_t, n, c["tiles_x"])["W"], 3)
        seen += got["counts"].sum(0)
    assert seen[0] and seen[1] and seen[5]


def hand_case():
    """one triangle, patch 2, one view of a 2 x 2 image, Z = 1 and the identity pose, so a point is given in pixels.  The four texels:
        (0, 0) weights  1 0 0  point 0.25 0.25  xs 64  ys 64   bilinear weights 36864 12288 12288  4096
        (1, 0) weights  0 1 0  point 0.75 0.25  xs 192 ys 64                    12288 36864  4096 12288
        (0, 1) weights  0 0 1  point 0.25 0.75  xs 64  ys 192                   12288  4096 36864 12288
        (1, 1) weights -1 1 1  point 0.75 0.75  xs 192 ys 192 (the gutter)       4096 12288 12288 36864"""
    img = np.array([[(10, 20, 30), (110, 120, 130)], [(50, 60, 70), (250, 240, 230)]], U8)[None]
    return mesh_case([(0.25, 0.25, 1), (0.75, 0.25, 1), (0.25, 0.75, 1)], [(0, 1, 2)], img)


HAND_SUMS = {(0, 0): [3358720, 3932160, 4505600], (1, 0): [7454720, 7864320, 8273920], (0, 1): [5488640, 5898240, 6307840], (1, 1): [11223040, 11141120, 11059200]}
HAND_BYTES = {(0, 0): [51, 60, 69], (1, 0): [114, 120, 126], (0, 1): [84, 90, 96], (1, 1): [171, 170, 169]}      # 51.25 60.0 68.75; 113.75 120.0 126.25; ...


def test_hand_case():
    c = hand_case()
    assert TM.texels_loop(2) == [(0, 0, 1, 0, 0), (1, 0, 0, 1, 0), (0, 1, 0, 0, 1), (1, 1, -1, 1, 1)]
    pts = TM.mix(c["vertices"], c["triangles"].astype(np.int64), 2)
    assert pts.tolist() == [[0.25, 0.25, 1], [0.75, 0.25, 1], [0.25, 0.75, 1], [0.75, 0.75, 1]]
    wts = {64: (192, 64), 192: (64, 192)}
    px = {(0, 0): (10, 20, 30), (1, 0): (110, 120, 130), (0, 1): (50, 60, 70), (1, 1): (250, 240, 230)}
    for (i, j), s in HAND_SUMS.items():
        (bx, ax), (by, ay) = wts[64 + 128 * i], wts[64 + 128 * j]
        assert s == [bx * by * px[0, 0][k] + ax * by * px[1, 0][k] + bx * ay * px[0, 1][k] + ax * ay * px[1, 1][k] for k in range(3)]
        assert HAND_BYTES[i, j] == [(x + 32768) >> 16 for x in s]
    for mode in ("mean", "best"):
        out = mirror(c, mode)
        want = np.zeros((4, 4, 3), U8)
        for (i, j), b in HAND_BYTES.items():
            want[j, i] = b
        assert out["atlas"].tolist() == want.tolist() and out["counts"].tolist() == [[0, 0, 0, 0, 0, 4]]
        assert out["views_used"].tolist() == [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
        state = np.frombuffer(out["state"][:128], np.uint64).reshape(4, 4)
        sums = [HAND_SUMS[0, 0], HAND_SUMS[1, 0], HAND_SUMS[0, 1], HAND_SUMS[1, 1]]
        assert state[:3].T.tolist() == ([[1024 * x for x in s] for s in sums] if mode == "mean" else sums)
        assert out["uv"].tolist() == [[[0.125, 0.875], [0.375, 0.875], [0.125, 0.625]]]
        assert same(out, loops(c, mode))
    best = mirror(c, "best")["best_view"]
    assert (best[:2, :2] == 0).all() and (best[2:] == 0xFFFFFFFF).all() and (best[:, 2:] == 0xFFFFFFFF).all()


# ---- the fallback and the arithmetic's edges -------------------------------------------------------------------------------------------------
def test_fallback_rounding_and_clamps():
    """patch 3 (D = 2), no view takes anything (the image lies beside the triangle).  Corner colours 0 255 255: the texel (1, 0) has
    q = 255, (2 * 255 + 2) // 4 = 128 (127.5 rounds up); the gutter texel (1, 2) has q = -0 + 255 + 510 = 765, 383 clamps to 255.
    Corner colours 255 0 0: (1, 0) has q = 255: 128; (1, 1) has q = 0; the gutter has q = -255: (-510 + 2) // 4 = -127 clamps to 0"""
    img = np.zeros((1, 2, 2, 3), U8)
    c = mesh_case([(50, 50, 1), (60, 50, 1), (50, 60, 1)], [(0, 1, 2)], img, patch=3)
    assert TM.texels_loop(3) == [(0, 0, 2, 0, 0), (1, 0, 1, 1, 0), (2, 0, 0, 2, 0), (0, 1, 1, 0, 1), (1, 1, 0, 1, 1), (2, 1, -1, 2, 1), (0, 2, 0, 0, 2), (1, 2, -1, 1, 2)]
    for corner, want in (((0, 255, 255), {(0, 0): 0, (1, 0): 128, (2, 0): 255, (0, 1): 128, (1, 1): 255, (2, 1): 255, (0, 2): 255, (1, 2): 255}),
                         ((255, 0, 0), {(0, 0): 255, (1, 0): 128, (2, 0): 0, (0, 1): 128, (1, 1): 0, (2, 1): 0, (0, 2): 0, (1, 2): 0}),
                         ((3, 4, 8), {(0, 0): 3, (1, 0): 4, (2, 0): 4, (0, 1): 6, (1, 1): 6, (2, 1): 7, (0, 2): 8, (1, 2): 9})):    # 3.5 -> 4, 5.5 -> 6, 6.5 -> 7, 8.5 -> 9
        cin = np.repeat(np.array(corner, U8)[:, None], 3, 1)
        for mode in ("mean", "best"):
            out = mirror(c, mode, colours_in=cin)
            assert out["counts"].tolist() == [[0, 8, 0, 0, 0, 0]] and not out["views_used"].any()
            got = {(i, j): int(out["atlas"][j, i, 0]) for (i, j) in want}
            assert got == want and (out["atlas"][..., 0] == out["atlas"][..., 2]).all()
            assert not out["atlas"][3:].any() and not out["atlas"][:, 3:].any() and same(out, loops(c, mode, cin))
            assert not mirror(c, mode)["atlas"].any()
    assert TM.fallback_loop(-1, 1, 2, 3, 255, 0, 0) == 0 and TM.fallback_loop(-1, 1, 2, 3, 0, 255, 255) == 255 and TM.fallback_loop(-1, 2, 1, 3, 1, 0, 0) == 0


@pytest.mark.parametrize("bad", [NAN, INF, -INF])
def test_a_non_finite_corner_gates_the_whole_triangle(bad):
    img = np.full((1, 8, 8, 3), 77, U8)
    for corner in range(3):
        for n in (2, 3, 6):
            v = np.array([(1, 1, 1), (6, 1, 1), (1, 6, 1), (6, 6, 1), (1, 6, 1), (6, 1, 1)], F)
            v[corner, 1] = bad
            c = mesh_case(v, [(0, 1, 2), (3, 4, 5)], img, patch=n)
            out = mirror(c)
            P = TX.layout(2, n)["texels_per_triangle"]
            assert out["counts"].tolist() == [[P, 0, 0, 0, 0, P]], (corner, n)        # the texels with weight 0 for the corner too
            assert same(out, loops(c)) and int((out["views_used"] != 0).sum()) == P


# ---- shared edges and the texture coordinates ------------------------------------------------------------------------------------------------
def test_a_shared_edge_has_equal_texels():
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (2, 24, 32, 3)).astype(U8)
    v = [(3.3, 2.1, 1), (27.9, 4.7, 1), (14.2, 21.6, 1), (17.1, -9.5, 1.0)]
    nrm = rng.normal(size=(4, 3)) * 0.2 + (0, 0, -1)
    for n in (2, 5, 6):
        c = mesh_case(v, [(0, 1, 2), (0, 1, 3)], img, normals=nrm, patch=n, R=EYE, t=np.array([[0, 0, 0], [0.1, 0, 0]]), min_cos=0.0)
        for mode in ("mean", "best"):
            out = mirror(c, mode)
            col, row = TM.atlas_pixels(2, n, 1)
            i, j, _, _, _ = TM.patch_texels(n)
            edge = np.flatnonzero((j == 0) & (i <= n - 1))                         # the texels of a - b: wc = 0, wa + wb = n - 1
            assert len(edge) == n
            for plane in ("atlas", "views_used"):
                first, second = out[plane][row[0, edge], col[0, edge]], out[plane][row[1, edge], col[1, edge]]
                assert first.tobytes() == second.tobytes()
            assert out["views_used"][row[0, edge], col[0, edge]].any()


def test_uv_closed_form_and_texel_centres():
    for n_t, n, tx in ((1, 2, 1), (5, 6, 2), (129, 14, 3), (7, 30, 1), (4, 3, 5)):
        L = TX.layout(n_t, n, tx)
        uv = TM.uv_of(n_t, n, tx)
        assert uv.dtype == F and uv.tobytes() == TM.uv_loop(n_t, n, tx).tobytes()
        col, row = TM.atlas_pixels(n_t, n, tx)
        i, j, _, _, _ = TM.patch_texels(n)
        corner = [int(np.flatnonzero((i == a) & (j == b))[0]) for a, b in ((0, 0), (n - 1, 0), (0, n - 1))]
        for t in range(n_t):
            for k in range(3):
                cx, ry = int(col[t, corner[k]]), int(row[t, corner[k]])
                assert uv[t, k, 0] == F((2 * cx + 1) / (2 * L["W"])) and uv[t, k, 1] == F((2 * (L["H"] - 1 - ry) + 1) / (2 * L["H"]))
                x, y = float(uv[t, k, 0]) * L["W"] - 0.5, (1.0 - float(uv[t, k, 1])) * L["H"] - 0.5
                assert abs(x - cx) < 1e-3 and abs(y - ry) < 1e-3
        assert ((uv > 0) & (uv < 1)).all()


# ---- a linear ramp ---------------------------------------------------------------------------------------------------------------------------
QUAD = [(12.3, 9.7, 1), (32.2, 11.1, 1), (30.9, 26.6, 1), (11.4, 25.2, 1)]      # a patch-2 gutter texel lies a whole leg past the hypotenuse: still in the image


def ramp_image(sx, sy, rows=48, cols=64, bump=None):
    y, x = np.mgrid[0:rows, 0:cols]
    img = 20.0 + sx * x + sy * y
    if bump is not None:
        img[bump] += 60.0
    assert img.min() >= 0 and img.max() <= 255                                  # unclipped
    return np.repeat(np.floor(img + 0.5).astype(U8)[None, :, :, None], 3, 3)


@pytest.mark.parametrize("slopes", [(2.0, 1.5), (0.5, -0.25), (-0.3, 2.0), (0.0, 0.0), (1.37, 0.61)])
@pytest.mark.parametrize("n", [2, 6, 14])
def test_linear_ramp_is_reproduced_by_a_bilinear_look_up(slopes, n):
    """the bound: half a grey level from the image's rounding carried through two convex combinations (the sample's and the look-up's) plus
    half a level from the atlas byte's rounding; the 1/256-pixel snap moves a sample by at most 1/512 pixel per axis; float32 slack"""
    sx, sy = slopes
    c = mesh_case(QUAD, [(0, 1, 2), (0, 2, 3)], ramp_image(sx, sy), patch=n)
    for mode in ("mean", "best"):
        out = mirror(c, mode)
        P = TX.layout(2, n)["texels_per_triangle"]
        assert out["counts"].tolist() == [[0, 0, 0, 0, 0, 2 * P]]
        rng = np.random.default_rng(n)
        bound = 1.0 + (abs(sx) + abs(sy)) / 512 + 0.01
        worst = 0.0
        for t, tri in enumerate(c["triangles"].tolist()):
            for b in rng.dirichlet((1, 1, 1), 150):
                p = b @ c["vertices"][tri].astype(np.float64)
                u, v = b @ out["uv"][t].astype(np.float64)
                got, _ = TM.lookup(out["atlas"], u, v)
                worst = max(worst, abs(got[0] - (20.0 + sx * p[0] + sy * p[1])))
        assert worst <= bound, (worst, bound)


def test_vertex_colours_cannot_hold_what_the_atlas_holds():
    """a ramp is linear, so four vertex colours interpolate it as well as the atlas does; what they cannot hold is anything between the
    vertices.  The same ramp with a 7 x 7 pixel block raised by 60 grey levels in a triangle's interior: the atlas texel whose point lies
    in the block shows it, the colour interpolated from the triangle's three recoloured vertices there is the ramp's"""
    sx, sy, n = 1.0, 0.5, 14
    img = ramp_image(sx, sy, bump=(slice(12, 19), slice(24, 31)))
    c = mesh_case(QUAD, [(0, 1, 2), (0, 2, 3)], img, patch=n)
    out = mirror(c)
    pts = TM.mix(c["vertices"], c["triangles"].astype(np.int64), n)
    col, row = TM.atlas_pixels(2, n, 1)
    inside = np.flatnonzero((np.abs(pts[:, 0] - 27) <= 2) & (np.abs(pts[:, 1] - 15) <= 2))
    assert len(inside) >= 1 and (inside < col.shape[1]).all()                      # texels of triangle 0
    vert = CM.recolour_numpy(c["vertices"], c["R"], c["t"], c["K"], c["rows"], c["cols"], c["colours"], **c["params"])["colours"].astype(np.float64)
    A, B, Cc = (c["vertices"][k].astype(np.float64) for k in c["triangles"][0])
    for e in inside:
        p = pts[e].astype(np.float64)
        ramp = 20.0 + sx * p[0] + sy * p[1]
        bary = np.linalg.solve(np.array([[A[0], B[0], Cc[0]], [A[1], B[1], Cc[1]], [1, 1, 1]]), [p[0], p[1], 1])
        from_vertices = bary @ vert[c["triangles"][0], 0]
        assert abs(from_vertices - ramp) <= 1.0 + (sx + sy) / 512 + 0.01 and abs(float(out["atlas"][row[0, e], col[0, e], 0]) - (ramp + 60.0)) <= 1.0 + (sx + sy) / 512 + 0.01


# ---- the Python layer, the header and the library -----------------------------------------------------------------------------------------
def test_argument_checkers_refuse_what_the_header_refuses():
    for f, good, bad in ((TX.patch_arg, (2, 6, 30, np.int64(5)), (1, 0, -1, 31, 6.0, True, "6", None)),
                         (TX.triangles_count_arg, (0, 1, (1 << 31) - 1), (-1, 1 << 31, 0.0, False, None)),
                         (lambda v: TX.capacity_arg(v, 16), (1, (1 << 31) - 1), (0, -1, 1 << 31, 1.0, True, None)),
                         (lambda v: TX.capacity_arg(1, v), (1, 1 << 28), (0, -1, (1 << 28) + 1, 16.0, None)),
                         (lambda v: TX.layout(10, 6, v), (1, 5, 2048, None), (0, -1, 2049, 1.0, True, "1")),
                         (TX.obj_paths, ("a.obj", "dir/b.OBJ"), ("a.ply", "a", ".obj", "dir/.obj"))):
        for v in good:
            f(v)
        for v in bad:
            with pytest.raises(ValueError):
                f(v)
    with pytest.raises(ValueError):
        TX.triangles_count_arg(11, 10)
    assert TX.obj_paths("x/y.obj") == ("x/y.obj", "x/y.mtl", "x/y.png")
    import torch
    host_v, host_t = torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32)
    for f, args in ((TX.mesh_arg, (host_v, host_t)), (TX.mesh_arg, (np.zeros((4, 3), F), host_t))):
        with pytest.raises(ValueError):
            f(*args)
    assert TX.MODES == RC.MODES and TX.COUNTS == CM.COUNTS and TX.NO_VIEW == 0xFFFFFFFF


def test_the_header_is_valid_c(tmp_path):
    src = tmp_path / "texture.c"
    src.write_text('#include "rgbid_texture.h"\nint main(void) { rgbid_texture_layout_t l; rgbid_recolour_params p; rgbid_recolour_view v; (void)l; (void)p; '
                   '(void)v; return sizeof l == 32 && sizeof p == 24 && sizeof v == 120 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "texture")])
    assert subprocess.run([str(tmp_path / "texture")]).returncode == 0
    text = open(os.path.join(ROOT, "include", "rgbid_texture.h")).read()
    assert f"RGBID_TEXTURE_MIN_PATCH {TX.MIN_PATCH}" in text and f"RGBID_TEXTURE_MAX_PATCH {TX.MAX_PATCH}" in text
    assert f"RGBID_TEXTURE_MAX_TRIANGLES {TX.MAX_TRIANGLES}ull" in text and f"RGBID_TEXTURE_MAX_TEXELS {TX.MAX_TEXELS}ull" in text
    assert '#include "rgbid_recolour.h"' in text and TM.MIN_PATCH == TX.MIN_PATCH and TM.MAX_PATCH == TX.MAX_PATCH and TM.MAX_DIM == TX.MAX_DIM
    for k in range(1, 9):
        assert f"\n *  {k}. " in text                                               # the contract's numbered steps


def test_the_library_exports_the_texture_functions():
    from tests.test_abi import _declared
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared("rgbid_texture.h")
    assert set(names) == set(TX.EXPORTS) and len(names) == 9
    assert not [n for n in names if not hasattr(L, n)]
    L = _lib.bind(TX.SIGNATURES)
    h, out, ms, lay = ctypes.c_void_p(), (ctypes.c_ulonglong * 6)(), (ctypes.c_float * 2)(), TX.Layout()
    p = RC.Params(0.05, 20.0, 0.02, 0.02, 0.2, 0)
    assert L.rgbid_texture_create(None, None, 10, 100) == -1 and L.rgbid_texture_create(ctypes.byref(h), None, 10, 100) == -1 and not h.value
    assert L.rgbid_texture_begin(None, 0, 6, 1, 0) == -1 and L.rgbid_texture_finish(None, None, None, 0, None, None, None) == -1
    assert L.rgbid_texture_add(None, None, None, 0, None, 0, 1, None, None, 4, 4, ctypes.byref(p)) == -1 and L.rgbid_texture_uv(None, None) == -1
    assert L.rgbid_texture_counts(None, 0, 1, out) == -1 and L.rgbid_texture_timing(None, 0, ms) == -1 and L.rgbid_texture_destroy(None) == 0
    assert L.rgbid_texture_layout(4, 6, 1, ctypes.byref(lay)) == 0 and (lay.T, lay.W, lay.H, lay.tiles, lay.tile_rows, lay.texels_per_triangle) == (8, 8, 16, 2, 2, 26)


def test_obj_round_trip(tmp_path):
    from rgbid import tum
    rng = np.random.default_rng(2)
    v = (rng.normal(size=(7, 3)) * 10.0 ** rng.uniform(-6, 6, (7, 1))).astype(F)
    nrm = rng.normal(size=(7, 3)).astype(F)
    tri = rng.integers(0, 7, (5, 3)).astype(U32)
    uv = TM.uv_of(5, 6, 2)
    atlas = rng.integers(0, 256, (16, 16, 3)).astype(U8)
    for normals in (None, nrm):
        path = tmp_path / ("n.obj" if normals is not None else "plain.obj")
        TX.write_obj(str(path), v, tri, uv, atlas, normals)
        got = TX.read_obj(str(path))
        assert got["vertices"].tobytes() == v.tobytes() and got["triangles"].tobytes() == tri.tobytes() and got["uv"].tobytes() == uv.tobytes()
        assert (got["normals"] is None) if normals is None else got["normals"].tobytes() == nrm.tobytes()
        stem = path.name[:-4]
        assert got["mtl"] == stem + ".mtl" and got["texture"] == stem + ".png" and got["atlas"].tobytes() == atlas.tobytes()
        assert tum.read_png(str(tmp_path / (stem + ".png"))).tobytes() == atlas.tobytes()
        text = path.read_text().splitlines()
        assert text[0] == f"mtllib {stem}.mtl" and sum(l.startswith("vt ") for l in text) == 15 and sum(l.startswith("f ") for l in text) == 5
        assert text[-1] == "f " + " ".join(f"{int(tri[4, k]) + 1}/{13 + k}" + (f"/{int(tri[4, k]) + 1}" if normals is not None else "") for k in range(3))
        assert f"map_Kd {stem}.png" in (tmp_path / (stem + ".mtl")).read_text()
    TX.write_obj(str(tmp_path / "empty.obj"), np.zeros((0, 3), F), np.zeros((0, 3), U32), np.zeros((0, 3, 2), F), np.zeros((8, 8, 3), U8))
    got = TX.read_obj(str(tmp_path / "empty.obj"))
    assert got["vertices"].shape == (0, 3) and got["triangles"].shape == (0, 3) and got["uv"].shape == (0, 3, 2) and got["atlas"].shape == (8, 8, 3)
    for kw in (dict(uv=uv[:4]), dict(normals=nrm[:6]), dict(atlas=atlas[:, :, 0]), dict(triangles=tri + 5), dict(path=str(tmp_path / "x.ply"))):
        args = dict(path=str(tmp_path / "bad.obj"), vertices=v, triangles=tri, uv=uv, atlas=atlas, normals=nrm)
        with pytest.raises(ValueError):
            TX.write_obj(**dict(args, **kw))


def test_command_line_option_errors(tmp_path):
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(tmp_path)]
    mesh = ["--mesh", str(tmp_path / "m.ply")]
    for extra, said in ((["--mesh-texture", str(tmp_path / "t.obj")], "--mesh-texture needs --mesh"),
                        (mesh + ["--mesh-texture-patch", "6"], "need --mesh-texture"),
                        (mesh + ["--mesh-texture-mode", "best"], "need --mesh-texture"),
                        (mesh + ["--mesh-texture-tolerance", "0.1"], "need --mesh-texture"),
                        (mesh + ["--mesh-texture-measured", "0.1"], "need --mesh-texture"),
                        (mesh + ["--mesh-texture", str(tmp_path / "t.obj"), "--mesh-texture-patch", "1"], "patch"),
                        (mesh + ["--mesh-texture", str(tmp_path / "t.obj"), "--mesh-texture-patch", "31"], "patch"),
                        (mesh + ["--mesh-texture", str(tmp_path / "t.obj"), "--mesh-texture-mode", "median"], "--mesh-texture-mode"),
                        (mesh + ["--mesh-texture", str(tmp_path / "t.obj"), "--mesh-texture-tolerance", "-1"], "--mesh-texture-tolerance"),
                        (mesh + ["--mesh-texture", str(tmp_path / "t.obj"), "--mesh-texture-measured", "nan"], "--mesh-texture-measured"),
                        (mesh + ["--mesh-texture", str(tmp_path / "t.ply")], "NAME.obj")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and said in r.stderr, (extra, r.stderr[-500:])
    assert not list(tmp_path.iterdir())
