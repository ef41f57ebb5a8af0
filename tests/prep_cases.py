"""The maps the frame-preparation stencils (csrc/kernels_prep.hip, csrc/kernels_bilateral.hip) are held to the oracle on: shapes at the wave, strip,
tile and grid boundaries of each kernel, and contents placed from the kernels' geometry.  Plain numpy: no GPU, no torch.

Kinds and their shapes (rows x cols of the SOURCE):
  pyr        k_pyr_down_dpp: 62 outputs per wave (lanes 0 / 63 are halo providers), 8 output rows per strip, 8-byte column pairs.  Source columns
             122..127, 248..251 (destination 61, 62, 63, 124, 125 columns, odd widths beside the even ones) at 16 and 33 rows; source rows 14..19, 32..35
             (destination 7, 8, 9, 16, 17 rows) at 124 and 251 columns; the tiny sources 2x2, 2x3, 3x2, 4x4, 5x5, 2x130.
  bil_fast   k_bilateral_shared / k_bilateral<2>: 60 outputs per wave (two halo lanes a side), 30 rows per wave below 32 lanes and 60 from 32 lanes on, four
             waves per workgroup, the step loop unrolled in threes.  Columns 1, 2, 3, 59, 60, 61, 119, 120, 121, 181 at 31 and 61 rows; rows 1..5, 29..33,
             59..61, 119..121 at 61 and 121 columns; 480x120 (8 tiles: renumbered by xcd_lane_local_tile) beside 480x121 (12: natural order).
  bil_fast32 the rows that matter at 60 rows per wave: 59, 60, 61, 62, 239, 240, 241 at 61 columns (run as 32 lanes).
  bil_exact  k_bilateral<0 | 1>, 64x16 tiles: columns 1, 63, 64, 65, 127, 128, 129 at 16 and 33 rows; rows 1, 15, 16, 17, 31, 32, 33 at 64 and 129 columns; 64x128
             (8 tiles) beside 64x129.
  sobel16    k_gradient4 / k_kf_maps4 (four pixels per thread, 8-row strips, 256 units per block): columns 4, 8, 60, 64, 68, 256 at 8 and 17 rows; rows 1, 2, 7,
             8, 9, 15, 16, 17 at 64 and 68 columns; 64 columns at 121, 128, 129 rows (16 units per strip: 256 units at 128 rows, one strip less and more).
  sobelfb    k_gradient (LDS tiles): columns 1, 2, 3, 63, 65, 66, 129 at 4 and 65 rows; rows 1, 3, 4, 5, 63, 64, 65 at 3 and 66 columns.
  prep       k_prep_frame4 (grid-stride, two units of four pixels per thread, 256 threads): cols x rows 4x511, 4x512, 4x513, 4x1024, 4x1025, 28x73, 8x128, 32x128
             (511, 512, 513, 1 024, 1 025, 511, 256, 1 024 units) and the three-kernel fallback at 30 columns.

Contents of a float map (Case.content):
  clean      no invalid pixel
  sparse     a clean map with ONE NaN, at a position taken from the kernel's geometry (sparse_positions): the case the pyramid's all-valid fast path
             exists for -- it switches on and off from wave to wave and row to row
  holes      the project's usual 10 % random NaN
  allnan     all NaN
  count      pyr only: interior windows with exactly 12 and exactly 13 valid taps (complement patterns of the 5x5 window, several layouts) and edge
             windows (15 taps) at 12 and 13; Case.meta lists (y, x, valid taps) of every planted window
  special    bil_fast only: +-1e9, 9.9e8, -9.9e8, +-inf, 1e19 among valid values; the FAST class's stated domain is the oracle on sanitised(map)
"""
import collections
import functools

import numpy as np

from tests import util

Case = collections.namedtuple("Case", "name kind rows cols content map meta")

PD_WAVE_OUT, PD_ROWS = 62, 8
BS_OUT = 60
BIL_MAXABS = 1e9


def _union(cols_list, at_rows, rows_list, at_cols, extra=()):
    s = [(r, c) for c in cols_list for r in at_rows] + [(r, c) for r in rows_list for c in at_cols] + list(extra)
    return tuple(dict.fromkeys(s))


SHAPES = {
    "pyr": _union((122, 123, 124, 125, 126, 127, 248, 249, 250, 251), (16, 33), (14, 15, 16, 17, 18, 19, 32, 33, 34, 35), (124, 251),
                  ((2, 2), (2, 3), (3, 2), (4, 4), (5, 5), (2, 130))),
    "bil_fast": _union((1, 2, 3, 59, 60, 61, 119, 120, 121, 181), (31, 61), (1, 2, 3, 4, 5, 29, 30, 31, 32, 33, 59, 60, 61, 119, 120, 121), (61, 121),
                       ((480, 120), (480, 121))),
    "bil_fast32": tuple((r, 61) for r in (59, 60, 61, 62, 239, 240, 241)),
    "bil_exact": _union((1, 63, 64, 65, 127, 128, 129), (16, 33), (1, 15, 16, 17, 31, 32, 33), (64, 129), ((64, 128), (64, 129))),
    "sobel16": _union((4, 8, 60, 64, 68, 256), (8, 17), (1, 2, 7, 8, 9, 15, 16, 17), (64, 68), ((121, 64), (128, 64), (129, 64))),
    "sobelfb": _union((1, 2, 3, 63, 65, 66, 129), (4, 65), (1, 3, 4, 5, 63, 64, 65), (3, 66)),
}
PREP_SHAPES = ((511, 4), (512, 4), (513, 4), (1024, 4), (1025, 4), (73, 28), (128, 8), (128, 32), (37, 30))   # rows, cols
PREP_DEPTHS = (0, 1, 9999, 10000, 10001, 65535)
# a view that starts one float into its allocation: the width is a multiple of 4, the base is not 16-byte aligned -- k_gradient, not k_gradient4
MISALIGNED_SHAPE = (17, 64)
EXACT_SIGMAS = (("W", 0.005), ("I", 3.0), ("W", 0.02))     # k_bilateral<1> at the tracker's two range sigmas, k_bilateral<0> at another
FAST_SIGMAS = (("W", 2 * 0.0025), ("I", 3.0))


def K_for(rows, cols):
    s = max(cols, 8) / 640.0
    return (525.0 * s, 525.0 * s, 319.5 * s, 239.5 * s)


def _seed(kind, rows, cols, extra=0):
    return 500000 + 7919 * sorted(SHAPES).index(kind) + 131 * rows + cols + 1000003 * extra


def base_map(kind, rows, cols, which="W", extra=0):
    """a clean map: inverse depth ("W") or intensity ("I")"""
    r = util.rng(_seed(kind, rows, cols, extra) + (17 if which == "I" else 0))
    return util.rand_invdepth(r, rows, cols, nan_frac=0.0) if which == "W" else util.rand_intensity(r, rows, cols)


def _pair_up(ys, xs):
    """every y and every x at least once, one position per map"""
    ys, xs = list(dict.fromkeys(ys)), list(dict.fromkeys(xs))
    if not ys or not xs:
        return ()
    n = max(len(ys), len(xs))
    return tuple(dict.fromkeys((ys[i % len(ys)], xs[i % len(xs)]) for i in range(n)))


def sparse_positions(kind, rows, cols):
    """-> ((y, x), ...) of the SOURCE map, from the kernel's geometry"""
    if kind == "pyr":
        # output row y of strip s = y // 8 reads source rows 2y - 2 .. 2y + 2: the first, a middle and the last output row of the first two strips
        ys = [2 * y + d for s in (0, 1) for y in (8 * s, 8 * s + 4, 8 * s + 7) for d in (-2, -1, 0, 1, 2)]
        # lane l of wave w owns the source column pair (2x, 2x + 1), x = 62 w + l - 1: lanes 0, 1, 62, 63 of waves 0 and 1, the even column only
        # and the odd column only
        xs = [2 * (PD_WAVE_OUT * w + l - 1) + odd for w in (0, 1) for l in (0, 1, 62, 63) for odd in (0, 1)]
    elif kind in ("bil_fast", "bil_fast32"):
        # a wave's first row is rpw * n and its last rpw * n + rpw - 1 (rpw = 30, or 60 from 32 lanes on): two above, one above, at, one below
        rpw = 60 if kind == "bil_fast32" else 30
        ys = [y + d for y in (0, rpw - 1, rpw, 2 * rpw - 1, 4 * rpw - 1, 4 * rpw) for d in (-2, -1, 0, 1)]
        xs = [BS_OUT * s + l - 2 for s in (0, 1, 2) for l in (0, 1, 2, 61, 62, 63)]      # lane l of strip s holds column 60 s + l - 2
    elif kind == "bil_exact":
        ys = [0, 1, 13, 14, 15, 16, 17, 18, 30, 31, 32]
        xs = [0, 1, 61, 62, 63, 64, 65, 66, 126, 127, 128]
    else:
        ys = [0, 1, 6, 7, 8, 9, 15, 16, rows - 2, rows - 1]
        xs = [0, 1, 3, 4, 7, 59, 60, 63, 64, 65, cols - 2, cols - 1]
    ys = [y for y in ys if 0 <= y < rows]
    xs = [x for x in xs if 0 <= x < cols]
    pos = _pair_up(ys, xs)
    if kind.startswith("sobel"):    # a NaN spreads to its 3x3 neighbourhood: keep the positions that leave a valid output
        pos = tuple((y, x) for y, x in pos if max(y, rows - 1 - y) > 1 or max(x, cols - 1 - x) > 1)
    return pos


def valid_taps(src):
    """valid taps of every pyramid window (clipped 5x5 around (2y, 2x)) -- integer work, independent of oracle and mirror"""
    rows, cols = src.shape[0] // 2, src.shape[1] // 2
    ok = np.pad(~np.isnan(src), 2, constant_values=False)
    n = np.zeros((rows, cols), int)
    for dy in range(5):
        for dx in range(5):
            n += ok[dy:dy + 2 * rows:2, dx:dx + 2 * cols:2]
    return n


def _window_patterns(r):
    """-> [(name, 5x5 bool VALID mask with 12 valid taps)]; its complement has 13"""
    yy, xx = np.mgrid[0:5, 0:5]
    pats = [("checker", (yy + xx) % 2 == 1)]
    top = np.zeros((5, 5), bool); top[:2] = True; top[2, :2] = True
    left = top.T.copy()
    ring = np.ones((5, 5), bool); ring[1:4, 1:4] = False; ring[0, 0] = ring[4, 4] = ring[0, 4] = ring[4, 0] = False
    pats += [("top", top), ("left", left), ("ring", ring)]
    for i in range(3):
        m = np.zeros(25, bool); m[r.choice(25, 12, replace=False)] = True
        pats.append((f"random{i}", m.reshape(5, 5)))
    assert all(int(p.sum()) == 12 for _, p in pats)
    return pats


def count_case(rows, cols):
    """a clean map with planted windows -> (map, ((y, x, valid taps), ...)) in DESTINATION coordinates.  Interior windows (25 taps in the image) get
    each pattern (12 valid) and its complement (13 valid); the left and the top edge (15 taps) get 3 and 2 invalid taps."""
    r = util.rng(_seed("pyr", rows, cols, 3))
    a = base_map("pyr", rows, cols, "W", 3)
    dr, dc = rows // 2, cols // 2
    pats = _window_patterns(r)
    plan = [(p, False) for _, p in pats] + [(p, True) for _, p in pats]
    # windows 6 apart are disjoint; interior ones start at source row / column 4, clear of the edge windows' rows / columns 0..2
    slots = [(y, x) for y in range(3, dr, 3) for x in range(3, dc, 3) if 2 * y + 2 < rows and 2 * x + 2 < cols]
    r.shuffle(slots)
    meta = []
    for i, (y, x) in enumerate(slots):
        p, comp = plan[i % len(plan)]
        valid = ~p if comp else p
        a[2 * y - 2:2 * y + 3, 2 * x - 2:2 * x + 3][~valid] = np.nan
        meta.append((y, x, int(valid.sum())))
    # edge windows: x = 0 keeps columns 0..2, y = 0 keeps rows 0..2 (15 taps); corners (9) can never reach 13
    k = 0
    for y in range(3, dr, 3):
        if 2 * y + 2 >= rows:
            continue
        n_bad = 3 if k % 2 == 0 else 2
        idx = r.choice(15, n_bad, replace=False)
        for j in idx:
            a[2 * y - 2 + j // 3, j % 3] = np.nan
        meta.append((y, 0, 15 - n_bad)); k += 1
    for x in range(3, dc, 3):
        if 2 * x + 2 >= cols:
            continue
        n_bad = 3 if k % 2 == 0 else 2
        idx = r.choice(15, n_bad, replace=False)
        for j in idx:
            a[j // 5, 2 * x - 2 + j % 5] = np.nan
        meta.append((0, x, 15 - n_bad)); k += 1
    return a, tuple(meta)


COUNT_SHAPES = ((16, 124), (33, 251), (35, 124), (19, 251))
SPECIALS = np.array([1e9, -1e9, 9.9e8, -9.9e8, np.inf, -np.inf, 1e19], np.float32)


def sanitised(a):
    """the FAST bilateral's stated domain: |v| >= 1e9 and +-inf count as invalid"""
    b = a.copy()
    with np.errstate(invalid="ignore"):
        b[~(np.abs(b) < BIL_MAXABS)] = np.nan
    return b


def special_case(kind, rows, cols, which):
    r = util.rng(_seed(kind, rows, cols, 5))
    a = base_map(kind, rows, cols, which, 5)
    n = max(SPECIALS.size, a.size // 25)
    idx = r.choice(a.size, min(n, a.size), replace=False)
    a.reshape(-1)[idx] = SPECIALS[np.arange(idx.size) % SPECIALS.size]
    if a.size >= 2 * SPECIALS.size:
        assert set(SPECIALS.tolist()) <= set(a.reshape(-1)[idx].tolist())
    return a


def _ro(a):
    a = np.ascontiguousarray(a, np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def float_cases(kind, which="W"):
    """-> (Case, ...) of one kind; `which`: inverse-depth ("W") or intensity ("I") values"""
    out = []
    for rows, cols in SHAPES[kind]:
        tag = f"{kind}-{rows}x{cols}-{which}"
        clean = base_map(kind, rows, cols, which)
        out.append(Case(tag + "-clean", kind, rows, cols, "clean", _ro(clean), None))
        for y, x in sparse_positions(kind, rows, cols):
            a = clean.copy(); a[y, x] = np.nan
            out.append(Case(f"{tag}-sparse@{y},{x}", kind, rows, cols, "sparse", _ro(a), (y, x)))
        h = base_map(kind, rows, cols, which, 1)
        h[util.rng(_seed(kind, rows, cols, 2)).random((rows, cols)) < 0.1] = np.nan
        out.append(Case(tag + "-holes", kind, rows, cols, "holes", _ro(h), None))
        out.append(Case(tag + "-allnan", kind, rows, cols, "allnan", _ro(np.full((rows, cols), np.nan, np.float32)), None))
        if kind in ("bil_fast", "bil_fast32"):
            out.append(Case(tag + "-special", kind, rows, cols, "special", _ro(special_case(kind, rows, cols, which)), None))
    if kind == "pyr":
        for rows, cols in COUNT_SHAPES:
            a, meta = count_case(rows, cols)
            out.append(Case(f"pyr-{rows}x{cols}-count", kind, rows, cols, "count", _ro(a), meta))
    return tuple(out)


def by_shape(cases):
    """-> {(rows, cols): [Case, ...]} in first-seen order"""
    d = {}
    for c in cases:
        d.setdefault((c.rows, c.cols), []).append(c)
    return d


# ---- keyframe maps: inverse depth with pixels on both sides of createNMapGradients' `acos_vn > 0.1` gate ---------------------------------------
def kf_gate_sides(w, K):
    """-> (pixels that pass the gate, pixels the gate alone rejects), by the float64 mirror"""
    from tests import np_mirror as M
    with np.errstate(all="ignore"):
        gx, gy = M.sobel(w)
        n = M.nmap_gradients(w, gx, gy, K)[0]
        defined = ~(np.isnan(w) | np.isnan(gx) | np.isnan(gy))
    return int(np.count_nonzero(defined & ~np.isnan(n))), int(np.count_nonzero(defined & np.isnan(n)))


@functools.lru_cache(maxsize=None)
def kf_cases():
    """sobel16 shapes: a smooth surface (normals face the camera) whose right half carries steep steps (they do not), 3 % NaN, plus one sparse and the all-NaN map of
    every shape.  The amplitude of the steps is the first of a fixed ladder at which the float64 mirror sees both sides of the gate in all three maps (asserted
    on the CPU)."""
    out = []
    for rows, cols in SHAPES["sobel16"]:
        K = K_for(rows, cols)
        r = util.rng(_seed("sobel16", rows, cols, 7))
        smooth = util.rand_invdepth(r, rows, cols, nan_frac=0.0)
        noise = r.uniform(-1.0, 1.0, (rows, cols)).astype(np.float32)
        noise[:, :cols // 2] = 0
        hole_mask = (r.random((rows, cols)) < 0.03) if rows * cols >= 64 else np.zeros((rows, cols), bool)
        y, x = sparse_positions("sobel16", rows, cols)[-1]
        for amp in (0.05, 0.1, 0.2, 0.4, 0.8, 1.6, 3.2):
            a = (smooth + np.float32(amp) * noise * smooth).astype(np.float32)
            holes = a.copy(); holes[hole_mask] = np.nan
            s = a.copy(); s[y, x] = np.nan
            if all(min(kf_gate_sides(m, K)) > 0 for m in (a, holes, s)):
                break
        out.append(Case(f"kf-{rows}x{cols}-gate", "kf", rows, cols, "gate", _ro(a), K))
        out.append(Case(f"kf-{rows}x{cols}-holes", "kf", rows, cols, "holes", _ro(holes), K))
        out.append(Case(f"kf-{rows}x{cols}-sparse@{y},{x}", "kf", rows, cols, "sparse", _ro(s), K))
        out.append(Case(f"kf-{rows}x{cols}-allnan", "kf", rows, cols, "allnan", _ro(np.full((rows, cols), np.nan, np.float32)), K))
    return tuple(out)


# ---- frame preparation ----------------------------------------------------------------------------------------------------------------------
PrepCase = collections.namedtuple("PrepCase", "name rows cols depth rgb")


@functools.lru_cache(maxsize=None)
def prep_cases():
    """u16 depth with 0, 1, 9 999, 10 000, 10 001 and 65 535 present (the clamp at 10 000 and the invalid 0), rgb with 0 and 255 in every channel"""
    out = []
    for rows, cols in PREP_SHAPES:
        r = util.rng(900000 + 131 * rows + cols)
        d = r.integers(0, 12000, (rows, cols)).astype(np.uint16)
        d[r.random((rows, cols)) < 0.1] = 0
        c = r.integers(0, 256, (rows, cols, 3)).astype(np.uint8)
        pos = r.choice(rows * cols, len(PREP_DEPTHS) + 8, replace=False)
        d.reshape(-1)[pos[:len(PREP_DEPTHS)]] = PREP_DEPTHS
        # the last pixel of the map and the four pixels of the first unit carry the clamp's neighbours too
        d[-1, -1] = 10001; d[0, :4] = (10000, 0, 65535, 9999)
        cf = c.reshape(-1, 3)
        for k in range(3):
            cf[pos[len(PREP_DEPTHS) + k], k] = 0
            cf[pos[len(PREP_DEPTHS) + 3 + k], k] = 255
        cf[pos[-2]] = 0; cf[pos[-1]] = 255
        d.setflags(write=False); c.setflags(write=False)
        out.append(PrepCase(f"prep-{rows}x{cols}", rows, cols, d, c))
    return tuple(out)
