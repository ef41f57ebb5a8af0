"""GPU tests of the keyframe segmenter (include/rgbid_segment.h, csrc/kernels_segment.hip, rgbid.segment): labels, counts, sizes,
histograms, mask levels and keypoint bits equal the sequential mirror (tests/segment_mirror.py), the negentropy image agrees to 2e-5 with
NaN in the same places, on the inputs of tests/test_cpu_segment.py, each with the default window and with windows of 1 and 64; a
keyframe gives the same bytes alone, inside a batch and from run to run; the mask_level option of rgbid.loopfeat.appearance_loops."""
import numpy as np
import pytest
import torch

from rgbid import loopfeat as LF
from rgbid import segment as SG
from tests import segment_mirror as SM
from tests.test_cpu_segment import K_OF, SIZES, TOL, mirror, near_threshold, scenes

pytestmark = pytest.mark.gpu
F = np.float32


def upload(block):
    return torch.from_numpy(np.ascontiguousarray(block)).cuda()


@pytest.fixture(scope="module")
def segmenters(ctx):
    made = {key: SG.Segmenter(ctx, *SIZES[key], 5, SIZES[key][0] * SIZES[key][1]) for key in ("a", "b")}   # the sizes of scenes()
    yield made
    for s in made.values():
        s.close()


def host(out):
    return [t.cpu().numpy() for t in out]


def assert_equals_mirror(name, got, member=0, m=None):
    """one keyframe of a device result against the mirror of scene `name` (or the mirror dict `m` of it, when the call did not use the
    scene's own parameters) -> the pixels a mask comparison skipped"""
    m = mirror(name) if m is None else m
    labels, counts, sizes, hist, neg, lev = [a[member] for a in got]
    c = m["count"]
    print(f"{name}: segments {counts} / {c}, edges {m['edges']}, levels {lev.tolist()} / {m['levels'].tolist()}")
    assert counts == c
    assert np.array_equal(labels, m["labels"])
    assert np.array_equal(sizes[:c], m["sizes"]) and not sizes[c:].any()
    assert np.array_equal(hist[:c], m["hist"]) and not hist[c:].any()
    assert np.array_equal(np.isnan(neg), np.isnan(m["negentropy"]))
    with np.errstate(invalid="ignore"):
        err = np.nanmax(np.abs(neg - m["negentropy"]), initial=0.0)
    print(f"{name}: negentropy error {err:.3g}")
    assert err <= TOL
    assert np.array_equal(lev, m["levels"])
    skip = near_threshold(m["negentropy"], m["valid"])
    assert skip.mean() <= 0.01
    assert np.array_equal(SM.masks_from_levels(neg, lev)[:, ~skip], SM.masks_from_levels(m["negentropy"], m["levels"])[:, ~skip])
    return skip


@pytest.mark.parametrize("name", sorted(scenes()))
def test_scene_equals_mirror_at_every_window(segmenters, name):
    s = scenes()[name]
    sg = segmenters[s["key"]]
    blk = upload(s["block"])
    rounds = {}
    try:
        for W in (SG.MAX_WINDOW, 1, 64):
            sg.set_window(W)
            got = host(sg.segment([blk], K_OF[s["key"]], k=s["kth"], min_size=s["min_size"]))
            assert_equals_mirror(name, got)
            rounds[W] = sg.last_rounds()
    finally:
        sg.set_window(SG.MAX_WINDOW)
    E = mirror(name)["edges"]
    print(f"{name}: rounds per pass {rounds}")
    assert rounds[1] == (E, E)                                   # a window of one decides one edge per round
    assert all(max(r) <= max(E, 1) for r in rounds.values())
    if E > 256:
        assert rounds[64][0] >= -(-E // 64) and rounds[SG.MAX_WINDOW][0] >= -(-E // 256)   # several windows ran


def test_batch_independence_and_determinism(segmenters):
    names = ["noisy_a", "flat", "holes", "nan_ny", "one_point"]     # five different keyframes of one size, default parameters
    sg = segmenters["a"]
    blks = [upload(scenes()[n]["block"]) for n in names]
    batch = host(sg.segment(blks, K_OF["a"], min_size=30))
    again = host(sg.segment(blks, K_OF["a"], min_size=30))
    alone = host(sg.segment([blks[3]], K_OF["a"], min_size=30))
    for a, b, c in zip(batch, again, alone):
        assert a.tobytes() == b.tobytes()
        assert a[3].tobytes() == c[0].tobytes()
    assert_equals_mirror("nan_ny", batch, member=3)                 # its scene runs at min_size = 30 too
    assert_equals_mirror("holes", batch, member=2)


def test_keypoint_bits_equal_mirror(segmenters):
    names = ["noisy_a", "holes", "k_zero"]
    sg = segmenters["a"]
    rows, cols = SIZES["a"]
    r = np.random.default_rng(21)
    cap = 96
    kps = np.zeros((3, cap), LF.KP_DTYPE)
    counts = np.array([cap, 50, 0], np.int32)
    kps["x"] = r.integers(0, cols, (3, cap)); kps["y"] = r.integers(0, rows, (3, cap))
    kps["x"][0, :4] = [-1, cols, 3, 5]; kps["y"][0, :4] = [2, 2, rows, -7]              # outside the image: level 0 only
    dk = torch.from_numpy(kps.view(np.uint8).reshape(3, cap, 120).copy()).cuda()
    dc = torch.from_numpy(counts).cuda()
    outs = []
    for n in names:                                                 # each scene has its own parameters: one call each, then stacked
        s = scenes()[n]
        outs.append(sg.segment([upload(s["block"])], K_OF["a"], k=s["kth"], min_size=s["min_size"]))
    neg = torch.cat([o[4] for o in outs]); lev = torch.cat([o[5] for o in outs])
    bits = sg.mask_keypoints(neg, lev, dk, dc).cpu().numpy()
    for i, n in enumerate(names):
        m = mirror(n)
        want = SM.keypoint_bits(m["negentropy"], m["levels"], list(zip(kps["x"][i, :counts[i]].tolist(), kps["y"][i, :counts[i]].tolist())))
        skip = near_threshold(m["negentropy"], m["valid"])
        sure = np.array([not (0 <= x < cols and 0 <= y < rows) or not skip[y, x] for x, y in zip(kps["x"][i, :counts[i]], kps["y"][i, :counts[i]])], bool)
        assert np.array_equal(bits[i, :counts[i]][sure], want[sure]) and not bits[i, counts[i]:].any()
    assert (bits[0, :4] == 1).all() and (bits & 1)[0].all()


def _keyframes(n, rows=120, cols=160):
    """a textured scene seen n times with a small shift: dict(frame, depthinv, colors, overlap_mask, normals) each"""
    from tests.test_cpu_segment import _noisy
    r = np.random.default_rng(8)
    tex = r.integers(0, 255, (rows // 4 + 8, cols // 4 + 8)).astype(np.uint8).repeat(4, 0).repeat(4, 1)
    depth, nrm = _noisy(rows, cols, 31, 0.3)
    nrm[:, :cols // 3] = np.array([0, 0, -1], F)                    # a featureless wall: low negentropy
    out = []
    for k in range(n):
        g = tex[2 * k:2 * k + rows, 3 * k:3 * k + cols]
        out.append(dict(frame=10 * k, depthinv=(F(1.0) / depth).astype(F), colors=np.ascontiguousarray(np.stack([g, g, g], -1)),
                        overlap_mask=np.zeros((rows, cols), np.uint8), normals=np.ascontiguousarray(np.moveaxis(nrm, -1, 0))))
    return out


def test_appearance_loops_mask_level(ctx, monkeypatch):
    kfs = _keyframes(5)
    K = (131.25, 131.25, 79.875, 59.875)
    base = LF.appearance_loops(ctx, kfs, K, max_keypoints=300, min_separation=1)
    called = []
    orig = LF.masked_features
    monkeypatch.setattr(LF, "masked_features", lambda *a, **kw: (called.append(1), orig(*a, **kw))[1])
    zero = LF.appearance_loops(ctx, kfs, K, max_keypoints=300, min_separation=1, mask_level=0)
    assert not called and zero[0] == base[0] and zero[2] == base[2]   # level 0 takes the path it took before: the same pairs, report
    assert all(a.tobytes() == b.tobytes() for ga, gb in zip(zero[1], base[1]) for a, b in zip(ga, gb))   # and guesses
    info = {}
    LF.appearance_loops(ctx, kfs, K, max_keypoints=300, min_separation=1, mask_level=2, mask_out=info)
    assert called
    lf = LF.LoopFeat(ctx, 120, 160, 300)
    try:
        from rgbid.posegraph import grey_from_colors
        kps, counts = lf.extract(np.stack([grey_from_colors(k["colors"]) for k in kfs]), np.stack([k["depthinv"] for k in kfs]), K).numpy()
    finally:
        lf.close()
    bits = info["bits"]
    assert counts.sum() > 0 and (info["counts"] < counts).any()     # the wall lost keypoints
    for i in range(len(kfs)):
        keep = ((bits[i, :counts[i]] >> 2) & 1).astype(bool)
        assert info["counts"][i] == keep.sum()
        assert info["kps"][i, :keep.sum()].tobytes() == kps[i, :counts[i]][keep].tobytes()      # every keypoint used has its bit 2 set
        assert not info["kps"][i, keep.sum():].view(np.uint8).any()
    with pytest.raises(ValueError):
        LF.appearance_loops(ctx, [{k: v for k, v in kf.items() if k != "normals"} for kf in kfs], K, max_keypoints=300, min_separation=1,
                            mask_level=1)                           # no blocks and nothing to build them from


def test_refusals_on_device(ctx, segmenters):
    sg = segmenters["a"]
    blk = upload(scenes()["flat"]["block"])
    for kw in (dict(k=-1.0), dict(k=float("nan")), dict(min_size=0), dict(nbins=0), dict(nbins=129), dict(levels=0), dict(levels=9)):
        with pytest.raises(Exception):
            sg.segment([blk], K_OF["a"], **kw)
    with pytest.raises(Exception):
        sg.segment([blk] * 6, K_OF["a"])                            # more than max_keyframes
    with pytest.raises(Exception):
        sg.set_window(0)
    with pytest.raises(Exception):
        sg.set_window(257)
    small = SG.Segmenter(ctx, *SIZES["a"], 1, 4)
    try:
        s = scenes()["k_zero"]
        with pytest.raises(ValueError):
            small.segment([upload(s["block"])], K_OF["a"], k=0.0, min_size=20)    # more segments than the tables hold
    finally:
        small.close()
