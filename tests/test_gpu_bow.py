"""GPU tests of the binary vocabulary (include/rgbid_bow.h, rgbid.bow) byte for byte against tests/bow_mirror.py: training over the set sizes
and shapes at which the kernels take another path (n = 0, 1, around k, one block, many blocks; uniform, clustered, equal and two-valued
sets; empty keyframes inside the batch), the weights, the transform (empty, single, full keyframes; one word; all weights zero; batch
independence), the score and the shortlist (exact ties, T above the candidates, pairs out of range), import / export."""
import numpy as np
import pytest
import torch

from rgbid import _lib
from rgbid import bow as BW
from rgbid import loopfeat as LF
from tests import bow_mirror as M
from tests.bow_cases import chunks, clustered, feats_of, uniform

pytestmark = pytest.mark.gpu
MAXKP = 1000


def trained(ctx, k, depth, per_kf, iters=10, max_kp=MAXKP):
    voc = BW.Vocabulary(ctx, k, depth)
    voc.train(feats_of(per_kf, max_kp), iters)
    return voc


def assert_tree(voc, desc, k, depth, what, iters=10):
    e = voc.export()
    cen, ch = M.train(desc, k, depth, iters)
    assert e["children"].shape == ch.shape and np.array_equal(e["children"], ch), (what, e["children"].shape, ch.shape)
    assert np.array_equal(e["centroids"], cen), what
    return e


@pytest.mark.parametrize("kind", ["uniform", "clustered"])
@pytest.mark.parametrize("k,depth", [(2, 1), (2, 3), (10, 1), (10, 3), (16, 1), (16, 3), (2, 6)])
def test_train_equals_the_mirror(ctx, k, depth, kind):
    r = np.random.default_rng(1000 * k + 10 * depth + (kind == "clustered"))
    voc = BW.Vocabulary(ctx, k, depth)
    try:
        for n in (0, 1, k - 1, k, k + 1, 1000, 20000):
            desc = uniform(r, n) if kind == "uniform" else clustered(r, n)
            voc.train(feats_of(chunks(desc)))
            e = assert_tree(voc, desc, k, depth, (k, depth, kind, n))
            print(f"k {k} depth {depth} {kind} n {n}: {len(e['children'])} nodes")
    finally:
        voc.close()


@pytest.mark.parametrize("k", [2, 10, 16])
def test_train_on_equal_and_two_valued_sets(ctx, k):
    r = np.random.default_rng(5)
    one, two = uniform(r, 1), uniform(r, 2)
    voc = BW.Vocabulary(ctx, k, 3)
    try:
        voc.train(feats_of(chunks(np.tile(one, (1000, 1)))))
        e = assert_tree(voc, np.tile(one, (1000, 1)), k, 3, "1 000 copies")
        assert len(e["children"]) == 1
        desc = np.tile(two, (500, 1))
        voc.train(feats_of(chunks(desc)))
        e = assert_tree(voc, desc, k, 3, "two descriptors 500 times each")
        assert len(e["children"]) == 3
    finally:
        voc.close()


def test_train_is_repeatable_and_ignores_empty_keyframes(ctx):
    r = np.random.default_rng(8)
    desc = clustered(r, 2500)
    voc = BW.Vocabulary(ctx, 10, 3)
    try:
        f = feats_of(chunks(desc))
        a = voc.train(f).export()
        b = voc.train(f).export()
        empty = np.zeros((0, 32), np.uint8)
        parts = [desc[:300], empty, desc[300:301], empty, empty, desc[301:1301], desc[1301:2301], empty, desc[2301:]]
        c = voc.train(feats_of(parts, seed=2)).export()
        for key in ("centroids", "children"):
            assert np.array_equal(a[key], b[key]) and np.array_equal(a[key], c[key]), key
        assert np.array_equal(a["weights"], b["weights"])
    finally:
        voc.close()


def test_weights_within_one_unit_of_the_mirror(ctx):
    r = np.random.default_rng(21)
    per_kf = [clustered(r, c) for c in (400, 0, 1000, 37, 650, 1)]
    voc = trained(ctx, 10, 2, per_kf)
    try:
        e = voc.export()
        words = [M.descend(e["centroids"], e["children"], d) for d in per_kf]
        want = M.weights(words, len(e["children"]))
        got = e["weights"]
        assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1
        assert (got[e["children"][:, 1] > 0] == 0).all() and (got > 0).any()
        # from another keyframe set; none at all zeroes them
        voc.set_weights(feats_of(per_kf[:3]))
        w3 = voc.export()["weights"]
        assert np.abs(w3.astype(np.int64) - M.weights(words[:3], len(w3)).astype(np.int64)).max() <= 1 and not np.array_equal(w3, got)
        voc.set_weights(feats_of([]))
        assert not voc.export()["weights"].any()
    finally:
        voc.close()


def test_transform_equals_the_mirror(ctx):
    mk = LF.MAX_KEYPOINTS
    r = np.random.default_rng(31)
    X, Y = uniform(r, 1), uniform(r, 1)
    base = [np.concatenate([clustered(r, 500), X]) for _ in range(4)]
    base[0] = np.concatenate([base[0], Y])
    voc = trained(ctx, 10, 3, base, max_kp=mk)
    try:
        e = voc.export()
        cen, ch, W = e["centroids"], e["children"], e["weights"]
        wx, wy = int(M.descend(cen, ch, X)[0]), int(M.descend(cen, ch, Y)[0])
        assert W[wx] == 0            # X is in every keyframe of the weight set
        batch = [np.zeros((0, 32), np.uint8), Y, clustered(r, mk), np.tile(Y, (40, 1)), np.tile(X, (7, 1))]
        f = feats_of(batch, mk, seed=3)
        bow = voc.transform(f, words=True)
        ent, cnt = bow.numpy()
        words = bow.words.cpu().numpy()
        for i, d in enumerate(batch):
            w = M.descend(cen, ch, d)
            assert np.array_equal(words[i, :len(d)], w) and (words[i, len(d):] == -1).all(), i
            v = M.vector(w, W)
            assert cnt[i] == len(v), (i, cnt[i], len(v))
            assert [(int(a), int(b)) for a, b in ent[i, :cnt[i]]] == v, i
            assert not ent[i, cnt[i]:]["word"].any() and not ent[i, cnt[i]:]["value"].any()
        assert cnt[0] == 0 and cnt[4] == 0 and cnt[2] > 100
        if W[wy]:
            assert cnt[1] == 1 and cnt[3] == 1 and ent[3, 0]["value"] == BW.ONE and ent[1, 0]["word"] == wy
        # a keyframe alone, and without the words output
        for i in (2, 3):
            one = voc.transform(LF.Features(f.kps[i:i + 1].contiguous(), f.counts[i:i + 1].contiguous()))
            e1, c1 = one.numpy()
            assert c1[0] == cnt[i] and np.array_equal(e1[0], ent[i])
    finally:
        voc.close()


def tied_keyframes(r, n=40):
    """keyframes drawn from a pool of 6 descriptor sets, so that many are identical and score exactly the same against any query"""
    pool = [clustered(r, int(c)) for c in (300, 280, 320, 150, 310, 5)]
    pick = r.integers(0, len(pool), n)
    return [pool[i] for i in pick], pick


def test_score_and_shortlist_equal_the_mirror(ctx):
    r = np.random.default_rng(41)
    per_kf, pick = tied_keyframes(r)
    n = len(per_kf)
    voc = trained(ctx, 10, 3, per_kf, max_kp=400)
    try:
        e = voc.export()
        f = feats_of(per_kf, 400)
        bow = voc.transform(f)
        vec = [M.vector(M.descend(e["centroids"], e["children"], d), e["weights"]) for d in per_kf]
        pairs = [(q, c) for q in range(n) for c in range(n)] + [(-1, 0), (0, n), (n, n), (3, -7)]
        got = voc.score(bow, pairs)
        want = np.array([M.score(vec[q], vec[c]) if 0 <= q < n and 0 <= c < n else 0 for q, c in pairs], np.uint64)
        assert np.array_equal(got, want)
        assert (got[-4:] == 0).all() and got[:n * n].max() <= BW.ONE
        ties = 0
        for sep in (1, 3):
            for T in (1, 8, 64):
                cand, sc = voc.shortlist(bow, sep, T)
                mc, ms = M.shortlist(vec, sep, T)
                assert np.array_equal(cand, mc) and np.array_equal(sc, ms), (sep, T)
                if T == 64:
                    assert (cand[:, n - sep:] == -1).all()        # T above the number of candidates: padded
                    ties += sum(1 for q in range(n) if len(set(sc[q][sc[q] > 0].tolist())) < int((sc[q] > 0).sum()))
        assert ties >= 6, ties
    finally:
        voc.close()


def test_export_import_round_trip_and_refusals(ctx, tmp_path):
    r = np.random.default_rng(51)
    per_kf = [clustered(r, 300) for _ in range(4)]
    voc = trained(ctx, 4, 3, per_kf, max_kp=300)
    other = BW.Vocabulary(ctx, 4, 3)
    try:
        e = voc.export()
        other.import_(e["centroids"], e["children"], e["weights"])
        o = other.export()
        for key in ("centroids", "children", "weights"):
            assert np.array_equal(e[key], o[key]), key
        f = feats_of(per_kf, 300)
        a, b = voc.transform(f).numpy(), other.transform(f).numpy()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        path = tmp_path / "voc.npz"
        voc.save(path)
        back = BW.load(ctx, path)
        assert back.k == 4 and back.depth == 3 and all(np.array_equal(back.export()[k_], e[k_]) for k_ in ("centroids", "children", "weights"))
        back.close()
        # a tree that is not numbered as the contract says, or is too deep or too wide for the handle, is refused and changes nothing
        bad = e["children"].copy(); bad[0, 0] = 2
        small = BW.Vocabulary(ctx, 4, 1)
        narrow = BW.Vocabulary(ctx, 2, 6)
        for h, ch in ((other, bad), (small, e["children"]), (narrow, e["children"])):
            with pytest.raises(_lib.RgbidError):
                h.import_(e["centroids"], ch, e["weights"])
        assert np.array_equal(other.export()["children"], e["children"])
        small.close(); narrow.close()
        with pytest.raises(_lib.RgbidError):
            voc.shortlist(voc.transform(f), 3, 65)
        with pytest.raises(_lib.RgbidError):
            voc.shortlist(voc.transform(f), 0, 8)
        with pytest.raises(_lib.RgbidError):
            BW.Vocabulary(ctx, 16, 6)
        # an untrained vocabulary is the root alone: every descriptor is word 0, of weight 0
        fresh = BW.Vocabulary(ctx, 10, 4)
        assert fresh.export()["children"].tolist() == [[0, 0]] and not fresh.transform(f).numpy()[1].any()
        fresh.close()
        t = voc.timing(True)
        voc.transform(f)
        assert set(voc.timing(False)) == set(BW.STAGES)
    finally:
        voc.close(); other.close()
