"""CPU tests of the keyframe segmenter (include/rgbid_segment.h): the two restatements of tests/segment_mirror.py (the sequential loop
and the reservation rounds) agree on every input the GPU tests use, for every window; the closed form of the mask rule equals the
replay of the reference's loops; the header is C; the library exports what it declares; the bin table agrees with numpy.  The inputs
(`scenes`) are export blocks built from synthetic depth and normals, shared with tests/test_gpu_segment.py.  `large_scenes` are the inputs
of tests/test_gpu_segment_large.py at 120 x 160 and 480 x 640: what the mirror alone says about them, and on which side of the device's
launch thresholds (csrc/voxel_device.h) the sizes of the large GPU tests lie."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import segment_mirror as SM
from tests.test_cpu_cloud import make_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TOL = 2e-5          # negentropy: at most 128 terms of at most 0.37 each, logf good to about 2 ULP, the divisor at least ln 2
SIZES = {"a": (37, 53), "b": (48, 64),     # both ragged against 64-lane tiles
         "c": (120, 160), "f": (480, 640)}  # the engine's export size and the full frame: large_scenes() only
K_OF = {"a": (45.0, 45.5, 26.0, 18.0), "b": (52.5, 52.5, 31.5, 23.5),
        "c": (131.25, 131.25, 79.875, 59.875), "f": (525.0, 525.0, 319.5, 239.5)}


def _lib_handle():
    from rgbid import _lib
    return ctypes.CDLL(_lib.LIB_PATH)


def _unit(n):
    with np.errstate(all="ignore"):
        return (n / np.sqrt((n * n).sum(-1, keepdims=True))).astype(F)


def _block(depth, normals):
    rows, cols = depth.shape
    with np.errstate(all="ignore"):
        iD = (F(1.0) / depth.astype(F)).astype(F)
    n = np.ascontiguousarray(np.moveaxis(normals.astype(F), -1, 0))       # planar
    return make_block(np.zeros(rows * cols, np.uint8), np.zeros((rows * cols, 3), np.uint8), iD, n)


def _plane(rows, cols):
    return np.ones((rows, cols), F), np.tile(np.array([0, 0, -1], F), (rows, cols, 1))


def _crease(rows, cols, slope, flip):
    """two planes meeting at the middle column; `flip` turns the normals to the other side (the sign of dot2)"""
    x = np.arange(cols, dtype=F)[None, :].repeat(rows, 0)
    depth = (1.0 + slope * np.abs(x - cols / 2) / cols).astype(F)
    s = np.where(x < cols / 2, -slope, slope).astype(F)
    n = _unit(np.stack([s, np.zeros_like(s), -np.ones_like(s)], -1))
    return depth, (-n if flip else n)


def _noisy(rows, cols, seed, amp=0.25):
    r = np.random.default_rng(seed)
    depth, n = _crease(rows, cols, 0.6, False)
    depth = (depth + 0.01 * r.standard_normal((rows, cols))).astype(F)
    return depth, _unit(n + amp * r.standard_normal((rows, cols, 3)).astype(F))


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> dict(size key, block, kth, min_size)"""
    out = {}

    def add(name, key, depth, n, kth=0.6, min_size=300, edit=None):
        depth, n = depth.copy(), n.copy()
        if edit:
            edit(depth, n)
        out[name] = dict(key=key, block=_block(depth, n), kth=kth, min_size=min_size)
    ra, ca = SIZES["a"]; rb, cb = SIZES["b"]
    add("flat", "a", *_plane(ra, ca))                                 # every weight ties: order by id alone
    add("crease", "a", *_crease(ra, ca, 0.8, False))
    add("convex", "a", *_crease(ra, ca, 0.1, False), min_size=50)         # 1 - dot = 0.02 at the crease: its square passes the threshold,
    add("concave", "a", *_crease(ra, ca, -0.1, False), min_size=50)       # the value itself does not (the sign of dot2)
    add("noisy", "b", *_noisy(rb, cb, 11), min_size=40)
    add("noisy_a", "a", *_noisy(ra, ca, 12, 0.1), min_size=25)

    def holes(depth, n):
        r = np.random.default_rng(5)
        depth[r.random(depth.shape) < 0.15] = np.nan
        n[r.random(depth.shape) < 0.1, 0] = np.nan
        depth[10:20, 8:30] = np.nan
    add("holes", "a", *_noisy(ra, ca, 13), min_size=30, edit=holes)

    def nothing(depth, n):
        depth[:] = np.nan
    add("no_point", "a", *_plane(ra, ca), edit=nothing)

    def one(depth, n):
        keep = depth[17, 29]
        depth[:] = np.nan
        depth[17, 29] = keep
    add("one_point", "a", *_plane(ra, ca), edit=one)

    def nan_ny(depth, n):
        n[9, 9, 1] = np.nan; n[30, 50, 1] = np.nan
    add("nan_ny", "a", *_noisy(ra, ca, 14), min_size=30, edit=nan_ny)   # dropped edges, points in no bin

    def id0(depth, n):
        depth[5, 5:9] = np.inf; depth[20, 40] = np.inf                  # iD = 0: d = inf, a point without a position
    add("id_zero", "a", *_noisy(ra, ca, 15), min_size=30, edit=id0)
    add("k_zero", "a", *_noisy(ra, ca, 16), kth=0.0, min_size=20)

    def islands(depth, n):
        for y, x in ((6, 6), (20, 31), (33, 47)):                       # single points behind a ring of invalid pixels
            keep = depth[y, x]
            depth[y - 1:y + 2, x - 1:x + 2] = np.nan
            depth[y, x] = keep
    add("min_one", "a", *_noisy(ra, ca, 17, 0.05), min_size=1, edit=islands)     # pass 2 does nothing
    add("min_all", "a", *_noisy(ra, ca, 18), min_size=ra * ca + 1, edit=holes)   # the connected components
    return out


def _faceted(rows, cols, cell, seed):
    """cells of cell x cell pixels, each a facet of its own normal unit((0.5 g1, 0.5 g2, -1)) at its own depth 1.5 + 0.05 g3; the noise on
    the normals is 0.03 times a factor of the facet's own (0.25 .. 4), so that the segments' entropies spread over the thresholds"""
    r = np.random.default_rng(seed)
    gy, gx = -(-rows // cell), -(-cols // cell)
    g = r.standard_normal((gy, gx, 3))
    amp = 0.03 * 2.0 ** r.uniform(-2.0, 2.0, (gy, gx))
    cy, cx = (np.arange(rows) // cell)[:, None], (np.arange(cols) // cell)[None, :]
    G, A = g[cy, cx], amp[cy, cx]
    depth = (1.5 + 0.05 * G[..., 2] + 0.002 * r.standard_normal((rows, cols))).astype(F)
    n = _unit(np.stack([0.5 * G[..., 0], 0.5 * G[..., 1], -np.ones((rows, cols))], -1))
    return depth, _unit(n + (A[..., None] * r.standard_normal((rows, cols, 3))).astype(F))


def _holes(seed):
    """15 % of the depths and 10 % of the normals' x NaN, and one NaN rectangle of a quarter by a third of the image"""
    def edit(depth, n):
        r = np.random.default_rng(seed)
        rows, cols = depth.shape
        depth[r.random(depth.shape) < 0.15] = np.nan
        n[r.random(depth.shape) < 0.1, 0] = np.nan
        depth[rows // 4:rows // 4 + rows // 4, cols // 8:cols // 8 + cols // 3] = np.nan
    return edit


FACETED = ("facets16", "facets5", "facets11_holes", "facets24_holes_f")


@functools.lru_cache(maxsize=None)
def large_scenes():
    """name -> dict(size key, block, kth, min_size) at the sizes past which the device's launches change shape (test_sizes_lie_on_the_
    intended_side_of_the_thresholds).  Not part of scenes(): the proofs over every window would take minutes here."""
    out = {}

    def add(name, key, depth, n, kth, min_size, edit=None):
        depth, n = depth.copy(), n.copy()
        if edit:
            edit(depth, n)
        out[name] = dict(key=key, block=_block(depth, n), kth=kth, min_size=min_size)
    rc, cc = SIZES["c"]; rf, cf = SIZES["f"]
    add("facets16", "c", *_faceted(rc, cc, 16, 41), kth=0.05, min_size=20)
    add("facets5", "c", *_faceted(rc, cc, 5, 42), kth=0.05, min_size=8)                 # hundreds of segments
    add("facets11_holes", "c", *_faceted(rc, cc, 11, 43), kth=0.05, min_size=20, edit=_holes(6))
    add("plane_c", "c", *_plane(rc, cc), kth=0.6, min_size=300)                          # every weight ties: about one round per point
    add("k_zero_c", "c", *_noisy(rc, cc, 44), kth=0.0, min_size=1)                      # every point its own segment: past DEFAULT_MAX_SEGMENTS
    add("facets24_holes_f", "f", *_faceted(rf, cf, 24, 45), kth=0.05, min_size=50, edit=_holes(7))
    return out


BATCH_SCENES = ("facets16", "facets5", "facets11_holes", "plane_c")     # the members of the 13- and 14-keyframe batches, cycled
BATCH_PARAMS = dict(kth=0.05, min_size=20)                               # one call has one set of parameters


@functools.lru_cache(maxsize=None)
def mirror(name, kth=None, min_size=None):
    """the mirror of a scene with its own parameters, or with the given ones"""
    s = scenes()[name] if name in scenes() else large_scenes()[name]
    rows, cols = SIZES[s["key"]]
    return SM.run(s["block"], rows, cols, K_OF[s["key"]], s["kth"] if kth is None else kth, s["min_size"] if min_size is None else min_size)


def near_threshold(neg, valid):
    """points whose negentropy lies within TOL of a threshold (pixels that are no point are exactly 0 on both sides)"""
    with np.errstate(invalid="ignore"):
        return valid.reshape(neg.shape) & (np.abs(neg[..., None] - SM.THRESHOLDS) <= TOL).any(-1)


def same_partition(r1, r2, valid):
    l1, c1 = SM.canonical(r1, valid); l2, c2 = SM.canonical(r2, valid)
    return c1 == c2 and np.array_equal(l1, l2)


@pytest.mark.parametrize("name", sorted(scenes()))
def test_rounds_equal_the_sequential_loop(name):
    s = scenes()[name]
    rows, cols = SIZES[s["key"]]
    valid, pos, nrm = SM.points(s["block"], rows, cols, K_OF[s["key"]])
    ids, ea, eb, ew = SM.edges(valid, pos, nrm, rows, cols)
    assert np.all(np.diff(ew) >= 0) and np.all((np.diff(ew) > 0) | (np.diff(ids) > 0))
    N = rows * cols
    seq = SM.segment_sequential(N, ea, eb, ew, s["kth"], s["min_size"])
    for W in (1, 7, 64, max(len(ea), 1)):
        rnd = SM.segment_rounds(N, ea, eb, ew, s["kth"], s["min_size"], W)
        assert same_partition(seq["root"], rnd["root"], valid), (name, W)
        assert same_partition(seq["root1"], rnd["root1"], valid), (name, W)
        assert np.array_equal(seq["size"][valid], rnd["size"][valid]) and np.array_equal(seq["size1"][valid], rnd["size1"][valid])
        assert np.array_equal(seq["th1"][valid].view(np.uint32), rnd["th1"][valid].view(np.uint32)), (name, W)
        assert max(rnd["rounds"]) <= max(len(ea), 1)
        if W == 1:
            assert rnd["rounds"] == (len(ea), len(ea))


def test_scenes_cover_the_cases():
    m = {n: mirror(n) for n in scenes()}
    assert m["no_point"]["count"] == 0 and m["no_point"]["edges"] == 0 and not m["no_point"]["negentropy"].any()
    assert m["one_point"]["count"] == 1 and np.isnan(m["one_point"]["negentropy"][17, 29])
    assert m["flat"]["count"] == 1 and m["flat"]["sizes"][0] == 37 * 53
    assert m["crease"]["count"] >= 2 and sorted((m["convex"]["count"], m["concave"]["count"])) == [1, 2]
    assert m["nan_ny"]["hist"].sum() == m["nan_ny"]["valid"].sum() - 2          # two points in no bin
    assert m["id_zero"]["edges"] == m["noisy_a"]["edges"]                       # dot2 is NaN there, the weight 1 - dot is not: no edge drops
    assert m["nan_ny"]["edges"] < m["noisy_a"]["edges"]                         # a NaN weight drops the edge
    assert (m["min_one"]["sizes"] == 1).any()                                   # pass 2 left single points
    assert m["min_all"]["count"] < m["holes"]["count"]
    assert m["k_zero"]["count"] > 10


@pytest.mark.parametrize("name", sorted(scenes()))
def test_mask_comparisons_are_decided_by_the_mirror_alone(name):
    """at most 1 % of the pixels lie within TOL of a threshold, and no such pixel can move a level: the GPU comparison of levels is exact"""
    m = mirror(name)
    neg = m["negentropy"]
    assert near_threshold(neg, m["valid"]).mean() <= 0.01
    for d in (-TOL, TOL):
        moved = np.where(m["valid"].reshape(neg.shape), neg + F(d), neg).astype(F)
        assert np.array_equal(SM.mask_levels(moved), m["levels"])


def _levels_are_decided(m):
    neg = m["negentropy"]
    assert near_threshold(neg, m["valid"]).mean() <= 0.01      # a condition on the input, not a tolerance: change the scene if it breaks
    for d in (-TOL, TOL):
        moved = np.where(m["valid"].reshape(neg.shape), neg + F(d), neg).astype(F)
        assert np.array_equal(SM.mask_levels(moved), m["levels"])


@pytest.mark.parametrize("name", sorted(large_scenes()))
def test_large_scenes_have_what_they_are_for(name):
    """from the mirror alone: the faceted scenes fill the segment tables, the plane is one segment of tied weights, k = 0 leaves more
    segments than the tables start with; and the levels are decided as in the small scenes"""
    m = mirror(name)
    rows, cols = SIZES[large_scenes()[name]["key"]]
    print(f"{name}: {m['count']} segments of {m['sizes'].min()} .. {m['sizes'].max()} points, {m['edges']} edges, levels {m['levels'].tolist()}")
    if name in FACETED:
        assert m["count"] >= 60 and m["sizes"].min() >= large_scenes()[name]["min_size"]
        assert len(np.unique(m["negentropy"][m["labels"] >= 0])) >= 30          # the segments' entropies differ
    elif name == "plane_c":
        assert m["count"] == 1 and m["sizes"][0] == rows * cols
    else:
        from rgbid import segment as SG
        assert name == "k_zero_c" and m["count"] > SG.DEFAULT_MAX_SEGMENTS == 4096
    if "holes" in name:
        assert 0.3 * 4 * rows * cols < m["edges"] < 0.6 * 4 * rows * cols and not m["valid"].all()
    else:
        assert m["edges"] == 4 * rows * cols - 3 * (rows + cols) + 2           # every pixel a point, no edge dropped
    _levels_are_decided(m)
    if name in BATCH_SCENES:
        b = mirror(name, **BATCH_PARAMS)
        assert b["count"] == 1 if name == "plane_c" else b["count"] >= 60
        _levels_are_decided(b)


def test_sizes_lie_on_the_intended_side_of_the_thresholds():
    """the sizes of the large GPU tests (tests/test_gpu_segment.py, tests/test_gpu_consist.py) against the constants of csrc/voxel_device.h:
    whoever retunes a constant learns here that those tests no longer reach the carried scans and the second trip of the strides"""
    txt = open(os.path.join(ROOT, "rgbid-slam_amd", "csrc", "voxel_device.h")).read()
    VT, SORT_IPT, RUN_IPT, MAX_GRID = (int(re.search(rf"constexpr int {n} = (\d+);", txt).group(1)) for n in ("VT", "SORT_IPT", "RUN_IPT", "VOX_MAX_GRID"))
    assert re.search(r"constexpr int SORT_TILE = VT \* SORT_IPT;", txt) and re.search(r"constexpr int RUN_TILE = VT \* RUN_IPT;", txt)
    assert len(re.findall(r"for \(unsigned base = 0; base < \w+; base \+= VT\)", txt)) == 2     # k_vox_scan_digits, k_vox_scan1: VT tiles per trip

    def tiles(items, per):
        return -(-items // per)
    P = SIZES["c"][0] * SIZES["c"][1]
    assert P == 19200 and SIZES["f"][0] * SIZES["f"][1] == 307200
    assert tiles(13 * 4 * P, VT * SORT_IPT) <= VT           # 244 sort tiles: one trip of k_vox_scan_digits
    assert tiles(14 * 4 * P, VT * SORT_IPT) > VT            # 263: the carry, 64-bit keys
    assert tiles(4 * 307200, VT * SORT_IPT) > VT            # 300: the carry, 32-bit keys
    assert P > 8 * VT                                       # k_seg_label carries over more than 8 tiles
    n = 524288
    assert tiles(n, VT) == MAX_GRID and tiles(n, VT * RUN_IPT) == VT          # exactly one grid, exactly one trip of k_vox_scan1
    assert tiles(n + 1, VT) == MAX_GRID + 1 and tiles(n + 1, VT * RUN_IPT) == VT + 1
    assert tiles(2 * n + 5003, MAX_GRID * VT) == 3          # three trips, the last one ragged


def test_mask_rule_closed_form_equals_the_replay():
    r = np.random.default_rng(3)
    imgs = []
    for i in range(8):
        imgs.append(r.random((9, 13)).astype(F) ** F(0.3 + 0.4 * i))
    imgs.append(np.full((6, 7), -1.0, F))                     # every pixel below every threshold, 0.f included: c_k is the whole image, no level satisfies the rule
    imgs.append(np.full((6, 7), 1.0, F))                      # nothing is ever masked: all levels take the last threshold
    imgs.append(np.zeros((6, 7), F))
    nan = r.random((8, 8)).astype(F); nan[2:5, 2:5] = np.nan
    imgs.append(nan)
    seen = set()
    for M in (1, 2, 4, 8):
        for neg in imgs:
            lev = SM.mask_levels(neg, M)
            assert np.array_equal(SM.masks_from_levels(neg, lev), SM.masks_replay(neg, M))
            seen.update(lev[1:].tolist())
    assert -1 in seen and 9 in seen and len(seen) > 4
    assert (SM.mask_levels(imgs[8], 4)[1:] == -1).all() and (SM.mask_levels(imgs[9], 4)[1:] == 9).all()


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_segment.c"
    src.write_text('#include "rgbid_segment.h"\n'
                   "typedef char window_is_256[RGBID_SEGMENT_MAX_WINDOW == 256 ? 1 : -1];\n"
                   "int use(rgbid_segment* s, float* c) { unsigned long long r[2];\n"
                   "  return rgbid_segment_bins(RGBID_SEGMENT_DEFAULT_BINS, c) + rgbid_segment_set_window(s, 1) + rgbid_segment_last_rounds(s, r); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_library_exports_segment_symbols():
    from rgbid import segment as SG
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_segment.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_segment_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(SG.EXPORTS), set(declared) ^ set(SG.EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing
    assert (SG.MAX_BINS, SG.MAX_LEVELS, SG.MAX_WINDOW) == tuple(int(re.search(rf"RGBID_SEGMENT_{n}\s+(\d+)", txt).group(1))
                                                                 for n in ("MAX_BINS", "MAX_LEVELS", "MAX_WINDOW"))


def test_bins_agree_with_numpy():
    from rgbid import segment as SG
    for nb in (1, 2, 80, 128):
        c = SG.bins(nb)
        assert c.shape == (nb, 3) and np.abs(c - SM.bins_numpy(nb)).max() <= 1e-6
        assert np.abs((c.astype(np.float64) ** 2).sum(1) - 1).max() < 1e-5
    L = _lib_handle()
    buf = (ctypes.c_float * 3)()
    assert L.rgbid_segment_bins(0, buf) == -1 and L.rgbid_segment_bins(129, buf) == -1 and L.rgbid_segment_bins(80, None) == -1


def test_refusals_and_sizing_before_any_device_call():
    from rgbid import segment as SG
    L = _lib_handle()
    h = ctypes.c_void_p(1)
    assert L.rgbid_segment_create(ctypes.byref(h), None, 48, 64, 1, 64) == -1 and not h.value
    b = ctypes.c_ulonglong()
    for bad in ((0, 64, 1, 1), (48, 64, 0, 1), (48, 64, 1, 0), (48, 64, 1, 48 * 64 + 1), (480, 640, 3496, 64)):
        assert L.rgbid_segment_workspace_bytes(*bad, ctypes.byref(b)) == -1, bad
    assert SG.workspace_bytes(480, 640, 3495, 64) > SG.workspace_bytes(480, 640, 256, 64) > 256 * 480 * 640 * 96
    assert L.rgbid_segment_set_window(None, 4) == -1 and L.rgbid_segment_destroy(None) == 0
