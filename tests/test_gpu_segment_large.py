"""GPU tests of the keyframe segmenter at the sizes it is used at (include/rgbid_segment.h, csrc/kernels_segment.hip, rgbid.segment): the
large scenes of tests/test_cpu_segment.py (120 x 160 and 480 x 640: tens to hundreds of segments, runs of 40 000 to 660 000 edges)
against the sequential mirror, held as tests/test_gpu_segment.py holds the small ones; batches of 13 and 14 keyframes, either side of
the carried scan of the sort's digit counts with 64-bit keys, and one 480 x 640 keyframe past it with 32-bit keys
(test_sizes_lie_on_the_intended_side_of_the_thresholds says which side each is on); tables that grow from the default to 19 200
segments; the engine's own exports."""
import numpy as np
import pytest
import torch

from rgbid import engine as E
from rgbid import segment as SG
from tests import segment_mirror as SM
from tests.test_cpu_cloud import make_block
from tests.test_cpu_segment import BATCH_PARAMS, BATCH_SCENES, K_OF, SIZES, TOL, large_scenes, mirror, near_threshold
from tests.test_gpu_cloud import K_SMALL, make_lanes
from tests.test_gpu_segment import assert_equals_mirror, host, upload

pytestmark = pytest.mark.gpu
F = np.float32
ROWS, COLS = SIZES["c"]


@pytest.fixture(scope="module")
def seg14(ctx):
    sg = SG.Segmenter(ctx, ROWS, COLS, 14, 4096)
    yield sg
    sg.close()


@pytest.fixture(scope="module")
def blocks_c():
    return {n: upload(s["block"]) for n, s in large_scenes().items() if s["key"] == "c"}


def run_scene(sg, name, blk, windows):
    """scene `name` alone at each window against its mirror -> {window: rounds per pass}"""
    s = large_scenes()[name]
    rounds = {}
    try:
        for W in windows:
            sg.set_window(W)
            got = host(sg.segment([blk], K_OF[s["key"]], k=s["kth"], min_size=s["min_size"]))
            assert_equals_mirror(name, got)
            rounds[W] = sg.last_rounds()
    finally:
        sg.set_window(SG.MAX_WINDOW)
    E_ = mirror(name)["edges"]
    print(f"{name}: {E_} edges, rounds per pass {rounds}")
    assert all(max(r) <= E_ for r in rounds.values())
    assert all(r[0] >= -(-E_ // W) for W, r in rounds.items())      # pass 1 saw every edge
    return rounds


@pytest.mark.parametrize("name", ["facets16", "facets5", "facets11_holes", "plane_c"])
def test_scene_of_export_size_equals_mirror(seg14, blocks_c, name):
    holed = name == "facets11_holes"
    rounds = run_scene(seg14, name, blocks_c[name], (SG.MAX_WINDOW, 64, 1) if holed else (SG.MAX_WINDOW,))
    E_ = mirror(name)["edges"]
    if holed:
        assert rounds[1] == (E_, E_)                                  # a window of one decides one edge per round
    if name == "plane_c":
        assert rounds[SG.MAX_WINDOW][0] >= ROWS * COLS // 4           # tied weights: the raster order chains the merges


def test_every_point_its_own_segment(ctx, blocks_c):
    """k = 0 and min_size = 1: 19 200 segments of one point, tables of exactly that many rows, every entropy 0 / 0"""
    m = mirror("k_zero_c")
    sg = SG.Segmenter(ctx, ROWS, COLS, 1, m["count"])
    try:
        run_scene(sg, "k_zero_c", blocks_c["k_zero_c"], (SG.MAX_WINDOW,))
    finally:
        sg.close()


def test_full_frame_equals_mirror(ctx):
    """one 480 x 640 keyframe: 1 228 800 edge slots, 300 sort tiles with 32-bit keys; tables of exactly the mirror's count"""
    name = "facets24_holes_f"
    m = mirror(name)
    sg = SG.Segmenter(ctx, *SIZES["f"], 1, m["count"])
    try:
        run_scene(sg, name, upload(large_scenes()[name]["block"]), (SG.MAX_WINDOW,))
    finally:
        sg.close()


def test_batches_either_side_of_the_sort_carry(seg14, blocks_c):
    """13 keyframes sort 244 tiles, 14 sort 263: one trip and two of the digit scan, 64-bit keys, keyframe indices up to 13 in the high
    word.  Every member equals its scene's mirror; the last member equals itself alone (the 32-bit path); a second run gives the same bytes."""
    K = K_OF["c"]
    kw = dict(k=BATCH_PARAMS["kth"], min_size=BATCH_PARAMS["min_size"])
    names13 = [BATCH_SCENES[(i + 1) % 4] for i in range(13)]          # the cycle starts at another scene
    names14 = [BATCH_SCENES[i % 4] for i in range(14)]
    got13 = host(seg14.segment([blocks_c[n] for n in names13], K, **kw))
    r13 = seg14.last_rounds()
    got14 = host(seg14.segment([blocks_c[n] for n in names14], K, **kw))
    r14 = seg14.last_rounds()
    again = host(seg14.segment([blocks_c[n] for n in names14], K, **kw))
    alone = host(seg14.segment([blocks_c[names14[13]]], K, **kw))
    for names, got in ((names13, got13), (names14, got14)):
        for i, n in enumerate(names):
            assert_equals_mirror(n, got, member=i, m=mirror(n, **BATCH_PARAMS))
    for a, b, c in zip(got14, again, alone):
        assert a.tobytes() == b.tobytes()
        assert a[13].tobytes() == c[0].tobytes()
    print(f"rounds per pass: 13 keyframes {r13}, 14 keyframes {r14}")
    assert r13 == r14                                                  # the same four scenes: the most rounds of a member


def test_tables_grow_from_the_default(ctx, blocks_c, monkeypatch):
    m = mirror("k_zero_c")
    created = []

    class Recording(SG.Segmenter):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            created.append(self.max_segments)
    monkeypatch.setattr(SG, "Segmenter", Recording)
    blk = blocks_c["k_zero_c"]
    s = large_scenes()["k_zero_c"]
    res = SG.segment_batches(ctx, [blk, blk, blk], K_OF["c"], ROWS, COLS, batch=2, max_segments=None, k=s["kth"], min_size=s["min_size"],
                             use=lambda sg, first, out: (sg.max_segments, [t.cpu().numpy() for t in out[:3]]))
    assert created == [SG.DEFAULT_MAX_SEGMENTS, m["count"]] and [S for S, _ in res] == [m["count"]] * 2
    assert [len(r[0]) for _, r in res] == [2, 1]
    for _, (labels, counts, sizes) in res:
        for k in range(len(labels)):
            assert counts[k] == m["count"] and np.array_equal(labels[k], m["labels"]) and np.array_equal(sizes[k], m["sizes"])


EXPORT_PARAMS = dict(kth=0.05, min_size=50)


def test_engine_exports_equal_mirror(ctx):
    """the engine's export ring -> keyframe_sources -> Segmenter against the mirror of the same keyframes read back through read_keyframe"""
    n, B = 9, 2
    seqs, depth, rgb = make_lanes(B, n, ROWS, COLS, K_SMALL, trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
    eng = E.Engine(ctx, E.default_config(rows=ROWS, cols=COLS, lanes=B, K=K_SMALL, record_capacity=n, keyframe_capacity=8, visratio_odo=0.985,
                                         visratio_integr=0.97))
    sg = None
    try:
        for k in range(n):
            eng.step(depth[k], rgb[k])
        counts = eng.keyframe_counts()
        assert (counts >= 2).all(), counts
        pairs = [(l, s) for l in range(B) for s in range(int(counts[l]))]
        srcs, _ = eng.keyframe_sources(pairs)
        kfs = [eng.read_keyframe(l, s) for l, s in pairs]
        sg = SG.Segmenter(ctx, ROWS, COLS, len(pairs), 4096)
        got = host(sg.segment(srcs, K_SMALL, k=EXPORT_PARAMS["kth"], min_size=EXPORT_PARAMS["min_size"]))
    finally:
        if sg is not None:
            sg.close()
        eng.close()
    print(f"engine exports: {len(pairs)} keyframes, segments {got[1].tolist()}")
    assert got[1].max() >= 2                                           # the tables hold more than one row somewhere
    worst, decided = 0.0, 0
    for i, a in enumerate(kfs):
        m = SM.run(make_block(a["overlap_mask"], a["colors"], a["depthinv"], a["normals"]), ROWS, COLS, K_SMALL, **EXPORT_PARAMS)
        labels, cnt, sizes, hist, neg, lev = [g[i] for g in got]
        c = m["count"]
        assert cnt == c and np.array_equal(labels, m["labels"])
        assert np.array_equal(sizes[:c], m["sizes"]) and not sizes[c:].any()
        assert np.array_equal(hist[:c], m["hist"]) and not hist[c:].any()
        assert np.array_equal(np.isnan(neg), np.isnan(m["negentropy"]))
        with np.errstate(invalid="ignore"):
            err = np.nanmax(np.abs(neg - m["negentropy"]), initial=0.0)
        worst = max(worst, float(err))
        assert err <= TOL
        assert np.array_equal(lev, SM.mask_levels(neg))                # the rule applied to the device's own image
        skip = near_threshold(m["negentropy"], m["valid"])
        if not skip.any():                                             # these inputs cannot be screened: the mirror's levels only then
            assert np.array_equal(lev, m["levels"])
            decided += 1
        assert np.array_equal(SM.masks_from_levels(neg, lev)[:, ~skip], SM.masks_from_levels(m["negentropy"], lev)[:, ~skip])
    print(f"engine exports: worst negentropy error {worst:.3g}, mirror's levels held on {decided} of {len(kfs)} keyframes")
