"""GPU tests of the binary vocabulary (include/rgbid_bow.h, rgbid.bow) on the block-level paths that tests/test_gpu_bow.py never enters, byte
for byte against tests/bow_mirror.py on the cases of tests/bow_cases.py (tests/test_cpu_bow_cases.py asserts on the CPU that each case has
the property it is there for):
  training   levels of more than 256 nodes (k_bow_finish_scan sums runs of 2 .. 16 nodes per thread; k_bow_seed_set and k_bow_finish_rows get
             further blocks), the default shape (10, 4) among them; Lloyd passes cut off at 1 and 2 and left to run to 64; keyframes shorter
             than a vote chunk; a handle trained on small sets after a large one; counts outside 0 .. max_keypoints
  transform  keyframe sizes on the edges of the bitonic sort and of the run-head chunks, 1 536 words in one keyframe, an entry of value 0
             under the largest weight training can produce; import refuses a larger one
  score and shortlist   hand-made vectors with which every wave of the shortlist meets more than the 64 candidates its list holds
The one tolerance is that of tests/test_gpu_bow.py: weights within one unit of the mirror's (the host's log is the only floating-point step)."""
import numpy as np
import pytest

from rgbid import _lib
from rgbid import bow as BW
from rgbid import loopfeat as LF
from tests import bow_cases as B
from tests import bow_mirror as M

pytestmark = pytest.mark.gpu


def assert_tree(e, tree, what):
    cen, ch = tree
    assert e["children"].shape == ch.shape and np.array_equal(e["children"], ch), (what, e["children"].shape, ch.shape)
    assert np.array_equal(e["centroids"], cen), what


def assert_weights(e, per_kf, what):
    """within one unit of the mirror's weights over the keyframes per_kf; nodes with children carry 0"""
    flat = M.descend(e["centroids"], e["children"], np.concatenate(per_kf)) if len(per_kf) else np.zeros(0, np.int32)
    words = np.split(flat, np.cumsum([len(d) for d in per_kf])[:-1]) if len(per_kf) else []
    want = M.weights(words, len(e["children"]))
    assert np.abs(e["weights"].astype(np.int64) - want.astype(np.int64)).max() <= 1, what
    assert not e["weights"][e["children"][:, 1] > 0].any(), what


def same_export(a, b):
    return all(a[key].shape == b[key].shape and np.array_equal(a[key], b[key]) for key in ("centroids", "children", "weights"))


@pytest.mark.parametrize("shape", B.TRAIN_SHAPES, ids=lambda s: "-".join(str(x) for x in s[:4]))
def test_train_with_levels_wider_than_a_block(ctx, shape):
    k, depth, n, kind, seed = shape
    desc = B.descriptors(n, kind, seed)
    voc = BW.Vocabulary(ctx, k, depth)
    try:
        e = voc.train(B.feats_of(B.chunks(desc))).export()
        assert_tree(e, B.mirror_tree(*shape), shape)
        assert max(B.split_levels(e["children"])) > B.BT
        assert_weights(e, B.chunks(desc), shape)
    finally:
        voc.close()


def test_default_vocabulary_is_the_first_shape(ctx):
    voc = BW.Vocabulary(ctx)
    try:
        assert (voc.k, voc.depth) == B.DEFAULT_SHAPE[:2] == (10, 4)
    finally:
        voc.close()


@pytest.mark.parametrize("iters", B.ITERS)
def test_train_with_lloyd_passes_cut_off_and_left_running(ctx, iters):
    k, depth, n, kind, seed = B.ITERS_SHAPE
    voc = BW.Vocabulary(ctx, k, depth)
    try:
        e = voc.train(B.feats_of(B.chunks(B.descriptors(n, kind, seed))), iters).export()
        assert_tree(e, B.mirror_tree(*B.ITERS_SHAPE, iters), iters)
        if iters < 64:       # the cut changed the tree, on the device too
            c64, h64 = B.mirror_tree(*B.ITERS_SHAPE, 64)
            assert not (e["centroids"].shape == c64.shape and np.array_equal(e["centroids"], c64) and np.array_equal(e["children"], h64))
    finally:
        voc.close()


def test_train_on_keyframes_shorter_than_a_vote_chunk(ctx):
    g = B.RAGGED
    batch = B.ragged_batch()
    desc = np.concatenate(batch)
    tree = M.train(desc, g["k"], g["depth"])
    voc = BW.Vocabulary(ctx, g["k"], g["depth"])
    try:
        ragged = voc.train(B.feats_of(batch, g["max_kp"], seed=5)).export()
        assert_tree(ragged, tree, "ragged")
        assert_weights(ragged, batch, "ragged")
        dense = voc.train(B.feats_of(B.chunks(desc), B.MAXKP, seed=6)).export()
        assert_tree(dense, tree, "dense")
        assert np.array_equal(ragged["centroids"], dense["centroids"]) and np.array_equal(ragged["children"], dense["children"])
    finally:
        voc.close()


def test_handle_trained_on_small_sets_after_a_large_one(ctx):
    k, depth, n, kind, seed = B.DEFAULT_SHAPE
    desc = B.descriptors(n, kind, seed)
    voc = BW.Vocabulary(ctx, k, depth)
    try:
        big = B.feats_of(B.chunks(desc))
        first = voc.train(big).export()
        assert_tree(first, B.mirror_tree(*B.DEFAULT_SHAPE), "first")
        for m in (11, 0, 1):
            e = voc.train(B.feats_of(B.chunks(desc[:m]))).export()
            assert_tree(e, M.train(desc[:m], k, depth), m)
            assert_weights(e, B.chunks(desc[:m]), m)
        assert len(voc.export()["children"]) == 1
        last = voc.train(big).export()
        assert same_export(first, last)
    finally:
        voc.close()


def test_counts_outside_the_range_read_as_its_ends(ctx):
    """a count below 0 reads as 0, one above max_keypoints as max_keypoints (include/rgbid_bow.h): train, set_weights and transform give the
    bytes of the batch that says so itself"""
    mk = 48
    r = np.random.default_rng(61)
    batch = [B.uniform(r, c) for c in (30, 20, mk, 0, mk, 17)]         # keyframe 1 is given -5, keyframe 4 mk + 7: its mk slots are real
    said = [len(d) for d in batch]
    said[1], said[4] = -5, mk + 7
    clamped = [batch[0], batch[1][:0], batch[2], batch[3], batch[4], batch[5]]
    f_out, f_in = B.feats_of(batch, mk, seed=7, counts=said), B.feats_of(clamped, mk, seed=7)
    a, b = BW.Vocabulary(ctx, 4, 3), BW.Vocabulary(ctx, 4, 3)
    try:
        ea, eb = a.train(f_out).export(), b.train(f_in).export()
        assert_tree(eb, M.train(np.concatenate(clamped), 4, 3), "clamped")
        assert same_export(ea, eb) and eb["weights"].any()
        wa, wb = a.set_weights(f_out).export()["weights"], b.set_weights(f_in).export()["weights"]
        assert np.array_equal(wa, wb)
        ta, tb = a.transform(f_out, words=True), b.transform(f_in, words=True)
        assert np.array_equal(ta.words.cpu().numpy(), tb.words.cpu().numpy())
        (enta, cnta), (entb, cntb) = ta.numpy(), tb.numpy()
        assert np.array_equal(enta, entb) and np.array_equal(cnta, cntb)
        words = ta.words.cpu().numpy()
        assert (words[1] == -1).all() and (words[4] >= 0).all() and cnta[1] == 0 and cnta[4] > 0
        assert np.array_equal(words[4], M.descend(eb["centroids"], eb["children"], batch[4]))
    finally:
        a.close(); b.close()


# ---- transform ----
def assert_vectors(bow, kfs, cen, ch, W, names):
    ent, cnt = bow.numpy()
    words = bow.words.cpu().numpy()
    for i, d in enumerate(kfs):
        w = M.descend(cen, ch, d)
        assert np.array_equal(words[i, :len(d)], w) and (words[i, len(d):] == -1).all(), names[i]
        v = M.vector(w, W)
        assert cnt[i] == len(v), (names[i], cnt[i], len(v))
        assert [(int(a), int(b)) for a, b in ent[i, :cnt[i]]] == v, names[i]
        assert not ent[i, cnt[i]:]["word"].any() and not ent[i, cnt[i]:]["value"].any(), names[i]
    return ent, cnt


def test_transform_on_the_sort_and_chunk_edges(ctx):
    k, depth, n, kind, seed = B.DEFAULT_SHAPE
    kfs, names = B.transform_batch()
    voc = BW.Vocabulary(ctx, k, depth)
    try:
        voc.train(B.feats_of(B.chunks(B.descriptors(n, kind, seed))))
        ws = B.weight_set()
        e = voc.set_weights(B.feats_of(ws)).export()
        assert_tree(e, B.mirror_tree(*B.DEFAULT_SHAPE), "transform vocabulary")
        assert_weights(e, ws, "weight set")
        cen, ch, W = e["centroids"], e["children"], e["weights"]
        f = B.feats_of(kfs, B.TRANSFORM_MAXKP, seed=3)
        ent, cnt = assert_vectors(voc.transform(f, words=True), kfs, cen, ch, W, names)
        i, c, t = names.index("distinct"), names.index("copies"), names.index("two_words")
        assert cnt[i] == 1536 and cnt[c] == 1 and ent[c, 0]["value"] == BW.ONE and cnt[t] == 2
        # the all-distinct keyframe alone, and without the words output
        one = voc.transform(LF.Features(f.kps[i:i + 1].contiguous(), f.counts[i:i + 1].contiguous()))
        e1, c1 = one.numpy()
        assert c1[0] == cnt[i] and np.array_equal(e1[0], ent[i])
    finally:
        voc.close()


def test_largest_weight_gives_an_entry_of_value_zero_that_stays(ctx):
    cen, ch, W, kfs = B.extreme_vocabulary()
    voc = BW.Vocabulary(ctx, 2, 1)
    try:
        assert BW.MAX_WEIGHT == B.MAX_WEIGHT == 726816
        voc.import_(cen, ch, W)                                        # 726 816 is accepted
        e = voc.export()
        assert np.array_equal(e["weights"], W) and np.array_equal(e["children"], ch) and np.array_equal(e["centroids"], cen)
        names = [str(p) for p in B.EXTREME_PAIRS]
        bow = voc.transform(B.feats_of(kfs, B.TRANSFORM_MAXKP, seed=4), words=True)
        ent, cnt = assert_vectors(bow, kfs, cen, ch, W, names)
        assert cnt.tolist() == [1, 2, 2, 1, 2]
        assert (int(ent[1, 1]["word"]), int(ent[1, 1]["value"])) == (2, 0) and ent[1, 0]["value"] == BW.ONE - 1      # value 0, and it stays
        vec = [M.vector(M.descend(cen, ch, d), W) for d in kfs]
        n = len(kfs)
        pairs = [(q, c) for q in range(n) for c in range(n)]
        got = voc.score(bow, pairs)
        assert np.array_equal(got, np.array([M.score(vec[q], vec[c]) for q, c in pairs], np.uint64))
        assert got[pairs.index((1, 0))] == 0 and got[pairs.index((0, 1))] == 0 and got[pairs.index((2, 0))] > 0
        cand, sc = voc.shortlist(bow, 1, 8)
        mc, ms = M.shortlist(vec, 1, 8)
        assert np.array_equal(cand, mc) and np.array_equal(sc, ms)
        assert (cand[1] == -1).all() and 0 in cand[2].tolist()         # the pair whose only common word has value 0 is no candidate
    finally:
        voc.close()


def test_import_refuses_weights_it_cannot_carry(ctx):
    cen, ch, W, kfs = B.extreme_vocabulary()
    voc = BW.Vocabulary(ctx, 2, 1)
    try:
        voc.import_(cen, ch, W)
        f = B.feats_of(kfs, B.TRANSFORM_MAXKP, seed=4)
        before = voc.transform(f).numpy()
        for bad, at in ((B.MAX_WEIGHT + 1, 1), (0xFFFFFFFF, 1), (B.MAX_WEIGHT + 1, 2), (0xFFFFFFFF, 0)):
            Wb = W.copy(); Wb[at] = bad
            with pytest.raises(_lib.RgbidError):
                voc.import_(cen ^ 0xFF, ch, Wb)
            e = voc.export()                                           # the former tree, centroids and weights included
            assert np.array_equal(e["weights"], W) and np.array_equal(e["children"], ch) and np.array_equal(e["centroids"], cen)
        after = voc.transform(f).numpy()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        # a trained handle likewise
        k, depth, n, kind, seed = B.ITERS_SHAPE
        tr = BW.Vocabulary(ctx, k, depth)
        try:
            e = tr.train(B.feats_of(B.chunks(B.descriptors(n, kind, seed)))).export()
            Wb = e["weights"].copy(); Wb[-1] = B.MAX_WEIGHT + 1
            with pytest.raises(_lib.RgbidError):
                tr.import_(e["centroids"], e["children"], Wb)
            assert same_export(tr.export(), e)
            Wb[-1] = B.MAX_WEIGHT
            assert tr.import_(e["centroids"], e["children"], Wb).export()["weights"][-1] == B.MAX_WEIGHT
        finally:
            tr.close()
    finally:
        voc.close()


# ---- score and shortlist on hand-made vectors ----
@pytest.fixture(scope="module")
def any_voc(ctx):
    """score and shortlist read the vectors alone: any vocabulary serves"""
    voc = BW.Vocabulary(ctx, 2, 1)
    yield voc
    voc.close()


@pytest.mark.parametrize("name", B.ALL_VECTOR_SETS)
def test_score_on_hand_made_vectors(any_voc, name):
    vec = B.vector_set(name)
    n = len(vec)
    r = np.random.default_rng(71)
    pairs = [tuple(p) for p in r.integers(0, n, (2000, 2)).tolist()] + [(n - 1, c) for c in range(n)] + [(-1, 0), (0, n), (n, n), (3, -7), (n - 1, -1)]
    got = any_voc.score(B.bow_of(vec), pairs)
    want = np.array([M.score(vec[q], vec[c]) if 0 <= q < n and 0 <= c < n else 0 for q, c in pairs], np.uint64)
    assert np.array_equal(got, want)
    assert (got[-5:] == 0).all() and got.max() <= BW.ONE and got.any()
    if name == "sparse":       # queries and candidates of count 0, 1 and 16 are among the pairs
        lens = {(len(vec[q]), len(vec[c])) for q, c in pairs[:-5]}
        assert {a for a, _ in lens} >= {0, 1, 16} and {b for _, b in lens} >= {0, 1, 16}


@pytest.mark.parametrize("name", B.ALL_VECTOR_SETS)
def test_shortlist_with_every_list_full(any_voc, name):
    vec = [list(v) for v in B.vector_set(name)]
    n = len(vec)
    bow = B.bow_of(vec)
    empty = [q for q in range(n) if not vec[q]]
    for sep, T in B.SHORTLIST_SETTINGS:
        cand, sc = any_voc.shortlist(bow, sep, T)
        mc, ms = M.shortlist(vec, sep, T)
        rows = np.flatnonzero((cand != mc).any(1) | (sc != ms).any(1))
        assert rows.size == 0, (name, sep, T, rows[:10], cand[rows[:1]], mc[rows[:1]])
        assert (cand[empty] == -1).all() and not sc[empty].any()
        if (sep, T) == (3, 64) and name in ("rising", "falling", "ties"):
            assert (cand[n - 1] >= 0).all()                            # the last query fills its 64 places
        if sep == 600:
            assert (cand == -1).all() and not sc.any()


def test_chain_on_many_small_keyframes(ctx):
    g = B.LOOP
    batch = B.loop_batch()
    voc = BW.Vocabulary(ctx, g["k"], g["depth"])
    try:
        f = B.feats_of(batch, g["per_kf"], seed=9)
        e = voc.train(f).export()
        assert_tree(e, M.train(np.concatenate(batch), g["k"], g["depth"]), "chain")
        assert_weights(e, batch, "chain")
        cen, ch, W = e["centroids"], e["children"], e["weights"]
        bow = voc.transform(f, words=True)
        assert_vectors(bow, batch, cen, ch, W, list(range(len(batch))))
        vec = [M.vector(M.descend(cen, ch, d), W) for d in batch]
        cand, sc = voc.shortlist(bow, g["min_separation"], g["T"])
        mc, ms = M.shortlist(vec, g["min_separation"], g["T"])
        assert np.array_equal(cand, mc) and np.array_equal(sc, ms)
        assert (cand[-1] >= 0).all()
    finally:
        voc.close()
