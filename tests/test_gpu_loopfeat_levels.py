"""GPU tests of the multi-level feature extractor (rgbid_loopfeat_create_levels / extract_levels / pyramid, rgbid.loopfeat) against the
numpy restatement tests/loopfeat_levels_mirror.py: every pyramid level, the 120-byte records, the 16-byte aux records and the counts byte for
byte; one level against the single-level entry points; batch independence; and a revisit at 1.6 x the distance end to end on the device
(match, RANSAC, gate, dense verifier), which one level loses and eight levels close."""
import ctypes as C

import numpy as np
import pytest
import torch

from rgbid import loopfeat as LF
from rgbid import posegraph as PG
from tests import loopfeat_levels_mirror as ML
from tests import loopfeat_mirror as M
from tests.test_gpu_loopfeat import K_of, textured

pytestmark = pytest.mark.gpu

SIZES = [(480, 640), (240, 320), (120, 160), (97, 131)]
POSE_BOUND = 4.1e-13          # 100 x the spread of the mirror's own two factorisations


def _degenerate(r, rows, cols):
    """random, constant, checkerboard, all 0, all 255"""
    yy, xx = np.mgrid[0:rows, 0:cols]
    return [r.integers(0, 256, (rows, cols)).astype(np.uint8), np.full((rows, cols), 77, np.uint8), (((yy + xx) & 1) * 255).astype(np.uint8),
            np.zeros((rows, cols), np.uint8), np.full((rows, cols), 255, np.uint8)]


@pytest.mark.parametrize("rows,cols", SIZES)
def test_pyramid_equals_mirror(ctx, rows, cols):
    """every level of 5 keyframes (random, constant, checkerboard, all 0, all 255) and of 1 keyframe equals the mirror's resize chain byte for
    byte; level 0 is the input; the library's level layout is the Python twin's"""
    r = np.random.default_rng(rows + cols)
    imgs = _degenerate(r, rows, cols)
    lf = LF.LoopFeat(ctx, rows, cols, 1000, 8, 1.2)
    try:
        plan = ML.budget(rows, cols, 1000, 8, 1.2)
        assert lf.levels == plan and [lf.level_layout(l) for l in range(len(plan))] == plan
        want = [ML.pyramid(g, plan) for g in imgs]
        for batch in (imgs, imgs[:1]):
            for l in range(len(plan)):
                got = lf.pyramid(np.stack(batch), l).cpu().numpy()
                assert got.shape == (len(batch), plan[l][0], plan[l][1])
                for k in range(len(batch)):
                    assert got[k].tobytes() == want[k][l].tobytes(), (rows, cols, l, k, int((got[k] != want[k][l]).sum()))
        with pytest.raises(ValueError):
            lf.pyramid(np.stack(imgs), len(plan))
    finally:
        lf.close()


def _assert_equal(feats, k, rec, aux, n, what):
    kps, counts = feats.numpy()
    ax = feats.numpy_aux()
    assert int(counts[k]) == n, (what, int(counts[k]), n)
    if kps[k].tobytes() != rec.tobytes():
        for i in range(len(rec)):
            assert kps[k][i].tobytes() == rec[i].tobytes(), (what, i, kps[k][i], rec[i], ax[k][i], aux[i])
    assert ax[k].tobytes() == aux.tobytes(), (what, [(i, ax[k][i], aux[i]) for i in range(len(aux)) if ax[k][i] != aux[i]][:3])


@pytest.mark.parametrize("rows,cols", SIZES)
@pytest.mark.parametrize("scale", [1.2, 1.5])
@pytest.mark.parametrize("levels", [1, 3, 8])
def test_records_equal_mirror(ctx, rows, cols, levels, scale):
    """records, aux records and counts equal the mirror's byte for byte; the depth maps have holes (NaN, 0, negative, inf), so the level-0
    depth predicate removes keypoints on the upper levels too"""
    r = np.random.default_rng(rows * 1000 + cols + levels)
    imgs = [textured(r, rows, cols) for _ in range(2)]
    K = K_of(rows, cols)
    tables = (M.rotated(), M.bounds())
    lf = LF.LoopFeat(ctx, rows, cols, 1000, levels, scale)
    try:
        feats = lf.extract(np.stack([g for g, _ in imgs]), np.stack([w for _, w in imgs]), K, aux=True)
        total, upper = 0, 0
        for k, (g, w) in enumerate(imgs):
            rec, aux, n = ML.extract(g, w, K, 1000, levels, scale, tables)
            _assert_equal(feats, k, rec, aux, n, (rows, cols, levels, scale, k))
            total += n; upper += int((aux["level"][:n] > 0).sum())
        print(f"{rows} x {cols}, {len(lf.levels)} of {levels} levels at {scale}: {total} keypoints over 2 images, {upper} on upper levels")
        assert total > 0
        assert feats.numpy()[0]["x"].max() < cols and feats.numpy()[0]["y"].max() < rows
    finally:
        lf.close()


def test_one_level_is_the_single_level_extractor(ctx):
    """an extractor from rgbid_loopfeat_create and one from rgbid_loopfeat_create_levels(..., 1, 1.2) give identical bytes on the images of the
    single-level feature test, through rgbid_loopfeat_extract and through rgbid_loopfeat_extract_levels"""
    L = LF._lib.lib()
    vp, ci = C.c_void_p, C.c_int
    L.rgbid_loopfeat_create.argtypes = [vp, vp, ci, ci, ci]
    L.rgbid_loopfeat_extract.argtypes = [vp, vp, vp, ci, vp, vp, vp]
    for rows, cols, max_kp in [(120, 160, 1000), (97, 131, 400), (64, 64, 256), (33, 40, 4), (240, 320, 1000)]:
        r = np.random.default_rng(rows * 1000 + cols)
        imgs = [textured(r, rows, cols) for _ in range(3)]
        K = K_of(rows, cols)
        lf = LF.LoopFeat(ctx, rows, cols, max_kp, 1, 1.2)
        h = C.c_void_p()
        LF.check(L.rgbid_loopfeat_create(C.byref(h), ctx._h, rows, cols, max_kp))
        try:
            feats = lf.extract(np.stack([g for g, _ in imgs]), np.stack([w for _, w in imgs]), K, aux=True)
            g = torch.from_numpy(np.stack([g for g, _ in imgs])).to(lf.dev)
            w = torch.from_numpy(np.stack([w for _, w in imgs])).to(lf.dev)
            kps = torch.empty((3, max_kp, 120), dtype=torch.uint8, device=lf.dev)
            counts = torch.zeros((3,), dtype=torch.int32, device=lf.dev)
            ctx.wait_torch_stream()
            LF.check(L.rgbid_loopfeat_extract(h, g.data_ptr(), w.data_ptr(), 3, (C.c_float * 4)(*K), kps.data_ptr(), counts.data_ptr()))
            ctx.sync()
            assert kps.cpu().numpy().tobytes() == feats.kps.cpu().numpy().tobytes()
            assert counts.cpu().numpy().tobytes() == feats.counts.cpu().numpy().tobytes()
            for k, (gi, wi) in enumerate(imgs):
                rec, n = M.extract(gi, wi, K, max_kp)
                assert int(feats.counts[k]) == n and feats.numpy()[0][k].tobytes() == rec.tobytes()
            ax = feats.numpy_aux()
            kp = feats.numpy()[0]
            assert not ax["level"].any() and np.array_equal(ax["lx"], kp["x"]) and np.array_equal(ax["ly"], kp["y"])
            assert lf.timing_pyramid() == 0.0
        finally:
            ctx.sync()
            L.rgbid_loopfeat_destroy(h)
            lf.close()


def test_batch_independence(ctx):
    """keyframe k's records and aux records depend neither on the batch size nor on its position in the batch (the scratch grows in between)"""
    rows, cols = 120, 160
    r = np.random.default_rng(8)
    imgs = [textured(r, rows, cols) for _ in range(6)]
    K = K_of(rows, cols)
    lf = LF.LoopFeat(ctx, rows, cols, 1000, 8, 1.2)
    try:
        one = [lf.extract(g[None], w[None], K, aux=True) for g, w in imgs[:2]]
        full = lf.extract(np.stack([g for g, _ in imgs]), np.stack([w for _, w in imgs]), K, aux=True)
        order = [4, 0, 5]
        part = lf.extract(np.stack([imgs[i][0] for i in order]), np.stack([imgs[i][1] for i in order]), K, aux=True)
        plain = lf.extract(np.stack([g for g, _ in imgs]), np.stack([w for _, w in imgs]), K)
        fk, fc = full.numpy(); fa = full.numpy_aux()
        assert plain.aux is None and plain.kps.cpu().numpy().tobytes() == full.kps.cpu().numpy().tobytes()
        with pytest.raises(ValueError):
            plain.numpy_aux()
        for k, f in enumerate(one):
            assert f.numpy()[1][0] == fc[k] and f.numpy()[0][0].tobytes() == fk[k].tobytes() and f.numpy_aux()[0].tobytes() == fa[k].tobytes()
        pk, pc = part.numpy(); pa = part.numpy_aux()
        for j, i in enumerate(order):
            assert pc[j] == fc[i] and pk[j].tobytes() == fk[i].tobytes() and pa[j].tobytes() == fa[i].tobytes()
        assert fc.min() > 0 and (fa["level"].max(axis=1) > 0).all()
    finally:
        lf.close()


def test_refusals_on_device(ctx):
    for bad in ((0, 1.2), (9, 1.2), (8, 1.0)):
        with pytest.raises(ValueError):
            LF.LoopFeat(ctx, 480, 640, 1000, *bad)
    with pytest.raises(ValueError):
        LF.LoopFeat(ctx, 480, 640, 900, 8, 1.2)
    L = LF._lib.lib()
    h = C.c_void_p()
    L.rgbid_loopfeat_create_levels.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]
    for levels, scale, mk in ((0, 1.2, 1000), (9, 1.2, 1000), (8, 1.0, 1000), (8, 1.2, 900)):
        assert L.rgbid_loopfeat_create_levels(C.byref(h), ctx._h, 480, 640, mk, levels, C.c_float(scale)) == -1 and not h.value


def test_levels_close_a_loop_that_one_level_loses(ctx):
    """The scale-change pair of tests/test_cpu_loopfeat_levels.py (the default scene at 320 x 240 from 0.75 m closer, depth ratio 1.59) on the
    device.  With 1 and with 8 levels: records equal the mirror's, the match list equals the mirror's, RANSAC's best iteration, inlier count
    and mask equal the mirror's (which flags neither case fragile) and its pose is within 4.1e-13 of the mirror's.  The reference's gate (10
    inliers, hull 0.05) fails with one level and passes with eight, and the dense verifier started from the RANSAC pose accepts the pair."""
    greys, ws, colors, (Rt, tt) = ML.scale_change_pair(0.75)
    rows, cols, K = ML.PAIR_ROWS, ML.PAIR_COLS, ML.PAIR_K
    tables = (M.rotated(), M.bounds())
    ok_by_levels = {}
    for levels in (1, 8):
        lf = LF.LoopFeat(ctx, rows, cols, 1000, levels, 1.2)
        try:
            feats = lf.extract(np.stack(greys), np.stack(ws), K, aux=True)
            want = [ML.extract(greys[k], ws[k], K, 1000, levels, 1.2, tables) for k in (0, 1)]
            for k in (0, 1):
                _assert_equal(feats, k, *want[k], ("pair", levels, k))
            pairs = [(1, 0)]                       # query: the closer view
            m, mc = lf.match(feats, pairs)
            res = lf.ransac(feats, pairs, m, mc)
            kps, _ = feats.numpy()
            mh = m.cpu().numpy().view(LF.MATCH_DTYPE).reshape(1, -1)[0, :int(mc[0])]
        finally:
            lf.close()
        g = ML.appearance_gate(want[0][0], want[0][2], want[1][0], want[1][2])
        mr = g["ransac"]
        assert mh.tobytes() == g["matches"].tobytes()
        assert not mr["fragile"]
        assert res["best"][0] == mr["best"] and res["inliers"][0] == mr["inliers"], (res["best"][0], res["inliers"][0], mr["best"], mr["inliers"])
        assert np.array_equal(res["mask"][0, :len(mh)], mr["mask"]) and not res["mask"][0, len(mh):].any()
        ok, inl, hq, hc = LF.gate(kps[1], kps[0], mh, res["mask"][0], rows, cols) if res["best"][0] >= 0 else (False, 0, 0.0, 0.0)
        print(f"levels {levels}: keypoints {want[0][2]}, {want[1][2]}; matches {len(mh)}; inliers {inl}; hull {hq:.3f} / {hc:.3f}; "
              f"gate {'passes' if ok else 'fails'}")
        assert (ok, inl) == (g["ok"], g["inliers"])
        if mr["best"] >= 0:
            dR, dt = float(np.abs(res["R"][0] - mr["R"]).max()), float(np.abs(res["t"][0] - mr["t"]).max())
            print(f"  device vs mirror pose: R {dR:.3e}, t {dt:.3e}; vs truth: t {np.linalg.norm(res['t'][0] - tt):.4f} m")
            assert dR <= POSE_BOUND and dt <= POSE_BOUND, (dR, dt)
        ok_by_levels[levels] = (ok, res["R"][0].copy(), res["t"][0].copy())
    assert not ok_by_levels[1][0] and ok_by_levels[8][0]
    _, Rr, tr = ok_by_levels[8]
    keyframes = [dict(frame=k, depthinv=ws[k], colors=colors[k]) for k in (0, 1)]
    Rs, ts = np.stack([np.eye(3)] * 2), np.zeros((2, 3))
    edges, report = PG.loop_constraints(ctx, keyframes, Rs, ts, K, pairs=[(1, 0)], guess=[(Rr, tr)])
    print("  dense verifier:", report)
    assert len(report) == 1 and report[0]["accepted"] and len(edges) == 1
