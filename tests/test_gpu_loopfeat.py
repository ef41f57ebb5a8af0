"""GPU tests of the loop-feature kernels (include/rgbid_loopfeat.h, rgbid.loopfeat) against the numpy restatement tests/loopfeat_mirror.py:
features and matches byte for byte (several sizes, degenerate images, batch independence), the RANSAC's choice exactly and its pose within
a bound derived from the mirror's own two factorisations, determinism."""
import numpy as np
import pytest
import torch

from rgbid import loopfeat as LF
from tests import loopfeat_mirror as M

pytestmark = pytest.mark.gpu

RANSAC_SEEDS = tuple(range(1000, 1064))     # 64 synthetic pairs; tests/test_cpu_loopfeat.py asserts that the mirror calls none of them fragile
GUARD = 1e-6
MAX_LEFT_OUT = 0.05


def textured(r, rows, cols, blobs=None):
    """a grey image with corners: random rectangles of random grey on a noisy background, and an inverse-depth map with invalid patches"""
    img = r.integers(90, 110, (rows, cols)).astype(np.int32)
    for _ in range(blobs if blobs is not None else rows * cols // 300):
        y, x = int(r.integers(0, rows - 4)), int(r.integers(0, cols - 4))
        h, w = int(r.integers(3, 24)), int(r.integers(3, 24))
        img[y:y + h, x:x + w] = int(r.integers(0, 256))
    w = r.uniform(0.3, 1.5, (rows, cols)).astype(np.float32)
    w[r.random((rows, cols)) < 0.05] = np.nan
    w[r.random((rows, cols)) < 0.02] = 0.0
    w[r.random((rows, cols)) < 0.01] = -0.5
    w[r.random((rows, cols)) < 0.01] = np.inf
    return img.clip(0, 255).astype(np.uint8), w


def K_of(rows, cols):
    return (1.1 * cols, 1.1 * cols, (cols - 1) / 2.0, (rows - 1) / 2.0)


def assert_features_equal(feats, k, rec, n, what):
    kps, counts = feats.numpy()
    assert int(counts[k]) == n, (what, int(counts[k]), n)
    a, b = kps[k].tobytes(), rec.tobytes()
    if a != b:
        for i in range(len(rec)):
            assert kps[k][i].tobytes() == rec[i].tobytes(), (what, i, kps[k][i], rec[i])
    assert a == b


@pytest.mark.parametrize("rows,cols,max_kp", [(120, 160, 1000), (97, 131, 400), (64, 64, 256), (33, 40, 4), (240, 320, 1000)])
def test_features_equal_mirror(ctx, rows, cols, max_kp):
    """records and counts equal the mirror's byte for byte; 97 x 131 and 33 x 40 are not multiples of the cell, 33 x 40 has one admissible row"""
    r = np.random.default_rng(rows * 1000 + cols)
    imgs = [textured(r, rows, cols) for _ in range(3)]
    K = K_of(rows, cols)
    lf = LF.LoopFeat(ctx, rows, cols, max_kp)
    try:
        feats = lf.extract(np.stack([g for g, _ in imgs]), np.stack([w for _, w in imgs]), K)
        total = 0
        for k, (g, w) in enumerate(imgs):
            rec, n = M.extract(g, w, K, max_kp)
            assert_features_equal(feats, k, rec, n, (rows, cols, k))
            total += n
        print(f"{rows} x {cols}: {total} keypoints over 3 images, per cell <= {lf.per_cell}")
        assert total > 0 or rows == 33
    finally:
        lf.close()


def test_features_degenerate_images(ctx):
    """a constant image, an image without a corner (a ramp), all-invalid depth: no keypoint, all records zero; and a valid one beside them"""
    rows, cols = 96, 128
    r = np.random.default_rng(5)
    g, w = textured(r, rows, cols)
    ramp = np.tile(np.arange(cols, dtype=np.uint8), (rows, 1))
    greys = [np.full((rows, cols), 77, np.uint8), ramp, g, g]
    ws = [np.ones((rows, cols), np.float32), np.ones((rows, cols), np.float32), np.full((rows, cols), np.nan, np.float32), w]
    K = K_of(rows, cols)
    lf = LF.LoopFeat(ctx, rows, cols, 500)
    try:
        feats = lf.extract(np.stack(greys), np.stack(ws), K)
        kps, counts = feats.numpy()
        assert list(counts[:3]) == [0, 0, 0] and counts[3] > 0
        assert not kps[:3].tobytes().strip(b"\0")
        for k in range(4):
            rec, n = M.extract(greys[k], ws[k], K, 500)
            assert_features_equal(feats, k, rec, n, k)
    finally:
        lf.close()


def _pair_set(r, rows, cols, n):
    """n keyframes of which neighbours share content (shifted copies), so that matches exist"""
    base, w = textured(r, rows + 40, cols + 40)
    greys, ws = [], []
    for k in range(n):
        dy, dx = int(r.integers(0, 40)), int(r.integers(0, 40))
        g = base[dy:dy + rows, dx:dx + cols].astype(np.int32) + r.integers(-3, 4, (rows, cols))
        greys.append(g.clip(0, 255).astype(np.uint8))
        ws.append(np.ascontiguousarray(w[dy:dy + rows, dx:dx + cols]))
    return greys, ws


def test_matches_equal_mirror_and_batch_independence(ctx):
    """match lists and counts equal the mirror's byte for byte (a keyframe without keypoints and one with a single keypoint among them); the
    same keyframe at another position of another batch gives the same records, and the same pair in another list the same matches"""
    rows, cols, max_kp = 120, 160, 600
    r = np.random.default_rng(11)
    greys, ws = _pair_set(r, rows, cols, 5)
    greys.append(np.full((rows, cols), 9, np.uint8)); ws.append(np.ones((rows, cols), np.float32))          # 5: no keypoint
    one = np.full((rows, cols), 100, np.uint8); one[50:70, 60:90] = 200
    wone = np.full((rows, cols), np.nan, np.float32); wone[50, 60] = 1.0                                        # 6: one keypoint at most
    greys.append(one); ws.append(wone)
    K = K_of(rows, cols)
    lf = LF.LoopFeat(ctx, rows, cols, max_kp)
    try:
        feats = lf.extract(np.stack(greys), np.stack(ws), K)
        kps, counts = feats.numpy()
        assert counts[5] == 0 and counts[6] <= 1
        pairs = [(1, 0), (2, 0), (4, 3), (3, 3), (0, 5), (5, 0), (0, 6), (6, 0), (4, 1)]
        m, mc = lf.match(feats, pairs)
        mh = m.cpu().numpy().view(LF.MATCH_DTYPE).reshape(len(pairs), max_kp)
        mch = mc.cpu().numpy()
        for k, (q, c) in enumerate(pairs):
            want = M.match(kps[q], counts[q], kps[c], counts[c])
            assert mch[k] == len(want), (q, c, mch[k], len(want))
            assert mh[k, :mch[k]].tobytes() == want.tobytes(), (q, c)
            assert not mh[k, mch[k]:].tobytes().strip(b"\0")
        assert list(mch[4:8]) == [0, 0, 0, mch[7]] and mch[0] > 10
        _, mc2 = lf.match(feats, pairs, lists=False)
        assert np.array_equal(mc2.cpu().numpy(), mch)
        # batch independence: other order, other batch size
        order = [4, 6, 0, 2]
        f2 = lf.extract(np.stack([greys[i] for i in order]), np.stack([ws[i] for i in order]), K)
        k2, c2 = f2.numpy()
        for j, i in enumerate(order):
            assert c2[j] == counts[i] and k2[j].tobytes() == kps[i].tobytes(), (j, i)
        m3, mc3 = lf.match(f2, [(0, 0), (2, 3), (0, 3)])           # (4, 4), (0, 2), (4, 2) of the first batch
        m4, mc4 = lf.match(feats, [(0, 2), (4, 2)])
        a, b = m3.cpu().numpy(), m4.cpu().numpy()
        assert np.array_equal(mc3.cpu().numpy()[1:], mc4.cpu().numpy()) and a[1].tobytes() == b[0].tobytes() and a[2].tobytes() == b[1].tobytes()
    finally:
        lf.close()


def _upload_synthetic(lf, pairs_data):
    """synthetic keypoint records and match lists -> (Features, pairs, matches tensor, counts tensor)"""
    P, mk = len(pairs_data), lf.max_keypoints
    kps = np.zeros((2 * P, mk), LF.KP_DTYPE)
    mt = np.zeros((P, mk), LF.MATCH_DTYPE)
    mc = np.zeros(P, np.int32)
    pairs = []
    for k, (kq, kc, m, _) in enumerate(pairs_data):
        kps[2 * k, :len(kq)] = kq
        kps[2 * k + 1, :len(kc)] = kc
        mt[k, :len(m)] = m
        mc[k] = len(m)
        pairs.append((2 * k, 2 * k + 1))
    dev = lf.dev
    feats = LF.Features(torch.from_numpy(kps.view(np.uint8).reshape(2 * P, mk, 120)).to(dev),
                        torch.from_numpy(np.array([len(p[0]) for p in pairs_data for _ in (0, 1)], np.int32)).to(dev))
    return feats, pairs, torch.from_numpy(mt.view(np.uint8).reshape(P, mk, 16)).to(dev), torch.from_numpy(mc).to(dev)


def synthetic_pairs(seeds=RANSAC_SEEDS):
    out = []
    for s in seeds:
        r = np.random.default_rng(s)
        out.append(M.synthetic_pair(r, n_good=int(r.integers(30, 90)), wrong=float(r.uniform(0.3, 0.7))))
    return out


def test_ransac_equals_mirror(ctx):
    """best iteration, inlier count and mask equal the mirror's on 64 synthetic pairs (30 - 70 % wrong matches); a pair is left out only when
    the mirror itself shows an error within 1e-6 of the threshold in a hypothesis within one inlier of its best, and at most 5 % are.
    qTc_ini: the mirror's SVD and Horn rotations disagree by at most `spread` on the best hypotheses; the device gets 100 x that.
    Measured on an MI355X: see DESIGN.md section 13."""
    data = synthetic_pairs()
    u = LF.uniform_draws(LF.num_iters())
    lf = LF.LoopFeat(ctx, 480, 640, 1000)
    try:
        feats, pairs, mt, mc = _upload_synthetic(lf, data)
        res = lf.ransac(feats, pairs, mt, mc)
        res2 = lf.ransac(feats, pairs, mt, mc, u=u)
        for key in res:
            assert res[key].tobytes() == res2[key].tobytes(), key
    finally:
        lf.close()
    left_out, spread, dev_R, dev_t, with_inliers = 0, 0.0, 0.0, 0.0, 0
    checked = []
    for k, (kq, kc, m, _) in enumerate(data):
        want = M.ransac(kq, kc, m, u, guard=GUARD)
        if want["fragile"]:
            left_out += 1
            continue
        assert res["best"][k] == want["best"] and res["inliers"][k] == want["inliers"], (k, res["best"][k], res["inliers"][k], want["best"], want["inliers"])
        assert np.array_equal(res["mask"][k, :len(m)], want["mask"]) and not res["mask"][k, len(m):].any(), k
        if want["best"] >= 0:
            with_inliers += 1
            spread = max(spread, float(np.abs(want["R"] - want["R_horn"]).max()), float(np.abs(want["t"] - want["t_horn"]).max()))
            checked.append((k, want))
            dev_R = max(dev_R, float(np.abs(res["R"][k] - want["R"]).max()))
            dev_t = max(dev_t, float(np.abs(res["t"][k] - want["t"]).max()))
    bound = 100.0 * spread
    print(f"ransac: {len(data)} pairs, {left_out} left out, {with_inliers} with a best hypothesis, inliers {res['inliers'].min()} .. {res['inliers'].max()}; "
          f"mirror SVD vs Horn {spread:.3e}, device vs mirror R {dev_R:.3e} t {dev_t:.3e}, bound {bound:.3e}")
    assert left_out <= MAX_LEFT_OUT * len(data)
    assert with_inliers >= len(data) // 2
    assert dev_R <= bound and dev_t <= bound, (dev_R, dev_t, bound)
    for k, want in checked:
        assert abs(np.linalg.det(res["R"][k]) - 1.0) < 1e-12


def test_ransac_few_matches_and_many_iterations(ctx):
    """fewer than 3 matches: no hypothesis (best -1, NaN pose, empty mask); more iterations than threads in a workgroup: still the mirror's"""
    r = np.random.default_rng(77)
    kq, kc, m, _ = M.synthetic_pair(r, 40, 0.4)
    data = [(kq, kc, m[:2], None), (kq, kc, m[:0], None), (kq, kc, m, None)]
    u = LF.uniform_draws(600, seed=123)
    lf = LF.LoopFeat(ctx, 480, 640, 1000)
    try:
        feats, pairs, mt, mc = _upload_synthetic(lf, data)
        res = lf.ransac(feats, pairs, mt, mc, u=u)
    finally:
        lf.close()
    assert list(res["best"][:2]) == [-1, -1] and list(res["inliers"][:2]) == [0, 0] and not res["mask"][:2].any()
    assert np.isnan(res["R"][:2]).all() and np.isnan(res["t"][:2]).all()
    want = M.ransac(kq, kc, m, u)
    assert not want["fragile"]
    assert res["best"][2] == want["best"] and res["inliers"][2] == want["inliers"] and np.array_equal(res["mask"][2, :len(m)], want["mask"])


def test_determinism(ctx):
    """two runs of every stage give the same bytes"""
    rows, cols, max_kp = 120, 160, 600
    outs = []
    for _ in range(2):
        r = np.random.default_rng(21)
        greys, ws = _pair_set(r, rows, cols, 4)
        lf = LF.LoopFeat(ctx, rows, cols, max_kp)
        try:
            feats = lf.extract(np.stack(greys), np.stack(ws), K_of(rows, cols))
            pairs = [(1, 0), (2, 1), (3, 0), (3, 2)]
            m, mc = lf.match(feats, pairs)
            res = lf.ransac(feats, pairs, m, mc)
            outs.append([feats.kps.cpu().numpy().tobytes(), feats.counts.cpu().numpy().tobytes(), m.cpu().numpy().tobytes(),
                         mc.cpu().numpy().tobytes()] + [res[k].tobytes() for k in sorted(res)])
        finally:
            lf.close()
    assert outs[0] == outs[1]
    assert np.frombuffer(outs[0][3], np.int32).max() > 10


def test_refusals_on_device(ctx):
    from rgbid._lib import RgbidError
    with pytest.raises(ValueError):
        LF.LoopFeat(ctx, 32, 64)
    with pytest.raises(ValueError):
        LF.LoopFeat(ctx, 480, 640, 100)
    lf = LF.LoopFeat(ctx, 64, 64, 100)
    try:
        feats = lf.extract(np.zeros((1, 64, 64), np.uint8), np.ones((1, 64, 64), np.float32), K_of(64, 64))
        with pytest.raises(RgbidError):
            lf.match(feats, [(0, 0)], ratio=float("nan"))
        with pytest.raises(RgbidError):
            lf.extract(np.zeros((1, 64, 64), np.uint8), np.ones((1, 64, 64), np.float32), (0.0, 1.0, 1.0, 1.0))
        m, mc = lf.match(feats, [(0, 7), (-1, 0)])      # keyframes that do not exist: no match, no fault
        assert list(mc.cpu().numpy()) == [0, 0]
        with pytest.raises(RgbidError):
            lf.ransac(feats, [(0, 0)], m, mc, u=np.zeros(3 * (LF.MAX_ITERS + 1)))
    finally:
        lf.close()
