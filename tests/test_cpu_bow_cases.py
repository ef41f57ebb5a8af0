"""Keeps the cases of tests/bow_cases.py honest before the GPU is held to tests/bow_mirror.py on them (tests/test_gpu_bow_paths.py): each
property below is what makes a case enter the path it is there for, asserted on the mirror alone.  No GPU, no library.

Measured here, and asserted:
  training shapes, nodes per level (LEVELS)
    (10, 4,  6 000, uniform)    [1, 10, 100, 1000, 5762]           split level of 1 000: per = ceil(N / 256) = 4, 250 busy threads
    (10, 4,  6 000, clustered)  [1, 10, 100, 622, 1538]            622: per 3, 208 busy threads, the last run holds 1 node
    ( 4, 6,  6 000, uniform)    [1, 4, 16, 64, 256, 1024, 3578]    1 024: per 4, every thread a full run
    (16, 4, 12 000, uniform)    [1, 16, 256, 4096, 11193]          4 096: per 16, every thread a full run
    (10, 4,  2 571, uniform)    [1, 10, 100, 1000, 2251]
    ragged batch (5 443 descriptors in 300 keyframes of at most 37, 28 empty)  [1, 10, 100, 1000, 5269]; 33 of its 174 vote chunks hold
    slots of three keyframes, 32 of them unused slots too
  iters: on uniform 3 000 at (10, 2) the trees at iters 1, 2, 3 and 10 all differ from the tree at 64
  candidates with S > 0 per wave (c mod 4) at min_separation 3: rising 149 .. 150 (last query), falling 147 .. 150 (each of the last ten
    queries), ties 119 .. 149, sparse 70 .. 92, the chain's 320 keyframes 70 .. 73: every wave's list of 64 fills and overflows
  rows of M.shortlist(v, 3, 64) a wrong kernel would get wrong, of 600 (MODEL_ROWS): four lists of 64 that stop inserting when full (and so
    keep the first 64 per wave to arrive): rising 341, ties 306; lists in which a newcomer behind all 64 keys takes the last lane instead of
    being dropped: none of falling (the best 64 of 256 keys never reach a list's last lane), queries 590 .. 592 of lone_wave, where wave 1
    alone holds candidates, 147 or 148 of them"""
import numpy as np
import pytest

from tests import bow_cases as B
from tests import bow_mirror as M

LEVELS = {
    (10, 4, 6000, "uniform"): [1, 10, 100, 1000, 5762],
    (10, 4, 6000, "clustered"): [1, 10, 100, 622, 1538],
    (4, 6, 6000, "uniform"): [1, 4, 16, 64, 256, 1024, 3578],
    (16, 4, 12000, "uniform"): [1, 16, 256, 4096, 11193],
    (10, 4, 2571, "uniform"): [1, 10, 100, 1000, 2251],
}
RAGGED_LEVELS = [1, 10, 100, 1000, 5269]
MODEL_ROWS = {"rising": 341, "ties": 306}


def per(N):
    return -(-N // B.BT)


def test_training_shapes_have_split_levels_wider_than_a_block():
    assert [s[:4] for s in B.TRAIN_SHAPES] == list(LEVELS)           # the shapes of the table, in its order
    wide = []
    for shape in B.TRAIN_SHAPES:
        _, ch = B.mirror_tree(*shape)
        sizes = B.level_sizes(ch)
        print(shape, sizes)
        assert sizes == LEVELS[shape[:4]], (shape, sizes)
        mine = [N for N in B.split_levels(ch) if N > B.BT]
        assert mine, shape
        wide += mine
    # runs of 2 or more nodes per thread: with every run full and with the last one cut short; with idle threads behind the last run
    assert any(per(N) >= 2 and N % per(N) == 0 for N in wide) and any(per(N) >= 2 and N % per(N) != 0 for N in wide)
    assert any(per(N) >= 2 and -(-N // per(N)) < B.BT for N in wide) and any(per(N) >= 2 and N == per(N) * B.BT for N in wide)
    assert {per(N) for N in wide} >= {3, 4, 16}
    assert {622, 1000, 1024, 4096} <= set(wide)
    # the default vocabulary's own shape is the first of the table
    assert B.DEFAULT_SHAPE[:2] == (10, 4)


def test_iters_cases_are_cut_off_before_convergence():
    trees = {it: B.mirror_tree(*B.ITERS_SHAPE, it) for it in (1, 2, 3, 10, 64)}
    assert B.ITERS == (1, 2, 64)
    for it in (1, 2, 3, 10):
        (cen, ch), (cen64, ch64) = trees[it], trees[64]
        assert not (cen.shape == cen64.shape and np.array_equal(cen, cen64) and np.array_equal(ch, ch64)), it


def test_ragged_batch_walks_keyframe_ends_and_unused_slots():
    g = B.RAGGED
    batch = B.ragged_batch()
    counts = [len(d) for d in batch]
    assert len(batch) == g["n_kf"] == 300 and g["max_kp"] == 37 and g["max_kp"] % B.VCHUNK and max(counts) == g["max_kp"]
    assert sum(c == 0 for c in counts) >= 20
    assert set(counts) == set(range(g["max_kp"] + 1))                # every count 0 .. 37 occurs
    census = B.chunk_census(counts, g["max_kp"])
    three = sum(1 for kfs, unused in census if kfs >= 3)
    both = sum(1 for kfs, unused in census if kfs >= 3 and unused > 0)
    print(f"ragged: {sum(counts)} descriptors, {sum(c == 0 for c in counts)} empty keyframes, {three} of {len(census)} vote chunks with slots of three "
          f"keyframes, {both} of them with unused slots")
    assert three >= 1 and both >= 1
    sizes = B.level_sizes(M.train(np.concatenate(batch), g["k"], g["depth"])[1])
    assert sizes == RAGGED_LEVELS, sizes


def test_transform_batch_sits_on_the_sort_and_chunk_edges():
    kfs, names = B.transform_batch()
    n = len(B.TRANSFORM_COUNTS)
    assert B.TRANSFORM_COUNTS == (1, 2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535, 1536)
    assert tuple(len(d) for d in kfs[:n]) == B.TRANSFORM_COUNTS and names[n:] == ["distinct", "copies", "two_words"]
    assert max(len(d) for d in kfs) == B.TRANSFORM_MAXKP == 1536
    cen, ch = B.mirror_tree(*B.DEFAULT_SHAPE)
    ws = B.weight_set()
    assert max(len(d) for d in ws) <= B.MAXKP
    words = [M.descend(cen, ch, d) for d in ws]
    W = M.weights(words, len(ch))
    held = np.unique(np.concatenate(words))
    assert np.array_equal(held, np.unique(M.descend(cen, ch, B.descriptors(*B.DEFAULT_SHAPE[2:]))))      # every word of the training set
    assert (W[held] > 0).all() and len(np.unique(W[held])) == 5                                         # no word is in every keyframe
    vec = {nm: M.vector(M.descend(cen, ch, d), W) for d, nm in zip(kfs, names)}
    assert len(vec["distinct"]) == 1536 and all(v > 0 for _, v in vec["distinct"])
    assert len(vec["copies"]) == 1 and vec["copies"][0][1] == B.ONE
    w2 = np.sort(M.descend(cen, ch, kfs[names.index("two_words")]))
    assert len(vec["two_words"]) == 2 and len(w2) == 600
    assert (w2[:300] == w2[0]).all() and (w2[300:] == w2[300]).all() and w2[0] < w2[300]        # the first run spans sorted index 255 | 256
    inp = M.descend(cen, ch, kfs[names.index("two_words")])
    assert inp[0] > inp[1]                                                                       # not sorted in the input
    # the counts around a power of two lead to word counts on both sides of it too: duplicates are few
    assert all(c - 50 <= len(vec[f"count {c}"]) <= c for c in B.TRANSFORM_COUNTS)


def test_extreme_weights_give_an_entry_of_value_zero():
    assert B.MAX_WEIGHT == int(np.floor(np.log(65535.0) * 65536.0 + 0.5)) == 726816
    assert 1536 * B.MAX_WEIGHT < 2 ** 31 and 1536 * (B.MAX_WEIGHT << 30) < 2 ** 64
    assert (1536 * 11184811) << 30 >= 2 ** 64            # where the shift would wrap (the header's bound leaves a factor of 15)
    cen, ch, W, kfs = B.extreme_vocabulary()
    assert W.tolist() == [0, 726816, 1] and [len(d) for d in kfs] == [7, 1536, 1536, 1536, 1536]
    vec = [M.vector(M.descend(cen, ch, d), W) for d in kfs]
    assert vec[0] == [(2, B.ONE)] and vec[3] == [(1, B.ONE)]
    assert len(vec[1]) == 2 and vec[1][1] == (2, 0) and vec[1][0][1] == B.ONE - 1         # count 2, the smaller entry is 0
    assert all(v > 0 for _, v in vec[2] + vec[4])
    assert M.score(vec[1], vec[0]) == 0 and M.score(vec[2], vec[0]) > 0
    cand, _ = M.shortlist(vec, 1, 8)
    assert 0 not in cand[1].tolist() and 0 in cand[2].tolist()


# ---- hand-made vectors ----
def wave_model(S, q, min_sep, T, drop):
    """k_bow_shortlist as it would be with one step wrong: four waves walk the candidates c = wave, wave + 4, ... of query q, each keeps a
    descending list of 64 keys (S, c).  drop = 'stop': a full list takes nothing more (it keeps the first 64 to arrive).  drop = 'never': a
    newcomer that ranks behind all 64 keys takes the last place instead of being dropped.  -> the T best keys over the four lists"""
    keys = []
    for wave in range(B.WAVES):
        mine = []
        for c in range(wave, q - min_sep + 1, B.WAVES):
            if S[q, c] == 0:
                continue
            x = (int(S[q, c]), c)
            if len(mine) == B.LANES and drop == "stop":
                continue
            pos = sum(1 for y in mine if y > x)
            if pos == B.LANES:
                if drop == "never":
                    mine[-1] = x
                continue
            mine.insert(pos, x)
            del mine[B.LANES:]
        keys += mine
    return sorted(keys, reverse=True)[:T]


def mirror_rows(name, min_sep=3, T=64):
    cand, sc = M.shortlist([list(v) for v in B.vector_set(name)], min_sep, T)
    return [[(int(s), int(c)) for s, c in zip(sc[q], cand[q]) if c >= 0] for q in range(len(cand))]


def test_vector_sets_are_well_formed():
    for name in B.ALL_VECTOR_SETS:
        v = B.vector_set(name)
        ent, cnt = B.pack_vectors(v)            # asserts ascending words and sums of at most ONE
        assert ent.shape == (B.VEC_N, B.VEC_MAXKP, 2) and len(v) == B.VEC_N == 600
        assert cnt.max() == (B.VEC_MAXKP if name == "sparse" else 4 if name == "ties" else 2)
    assert B.VECTOR_SETS == ("rising", "falling", "ties", "sparse")
    assert {len(v) for v in B.vector_set("sparse")} == set(range(0, 17))                      # counts 0, 1 and 16 among them
    assert sum(len(v) == 0 for v in B.vector_set("ties")) == 60 == sum(len(v) == 0 for v in B.vector_set("sparse"))
    S = B.score_table("sparse")
    lonely = [c for c in range(B.VEC_N) if c % 5 == 2]
    assert not (S + S.T)[lonely].any() and all(len(B.vector_set("sparse")[c]) for c in lonely)      # they share no word with anyone
    r = B.score_table("rising")
    assert all(r[q, c] == B.ONE - B.VEC_STEP * (q - c) for q in (1, 300, 599) for c in range(q))
    f = B.score_table("falling")
    assert all(f[q, c] == B.VEC_STEP * (600 - c) for q in range(590, 600) for c in range(590))
    t = B.score_table("ties")
    assert set(np.unique(t).tolist()) == {0, B.ONE // 4, B.ONE}


@pytest.mark.parametrize("name", B.VECTOR_SETS)
def test_every_wave_meets_more_candidates_than_its_list_holds(name):
    S = B.score_table(name)
    n = len(S)
    for q in (range(n - 10, n) if name == "falling" else [n - 1]):
        per_wave = [int((S[q, w:q - 2:B.WAVES] > 0).sum()) for w in range(B.WAVES)]
        print(name, "query", q, "candidates with S > 0 per wave at min_separation 3:", per_wave)
        assert min(per_wave) >= 65, (name, q, per_wave)


def test_ties_are_ordered_by_the_candidate_alone():
    rows = mirror_rows("ties")
    tied = sum(1 for row in rows if len({s for s, _ in row}) < len(row))
    print("ties: queries with two equal scores inside their top 64:", tied)
    assert tied >= 100


def test_a_kernel_that_mishandles_a_full_list_is_caught():
    """the models live here and not in the mirror: they are wrong on purpose"""
    for name in ("rising", "ties"):
        S, rows = B.score_table(name), mirror_rows(name)
        wrong = sum(1 for q in range(len(S)) if wave_model(S, q, 3, 64, "stop") != rows[q])
        print(f"{name}: four lists that stop inserting when full (the first 64 per wave to arrive) differ from the mirror on {wrong} of {len(S)} rows")
        assert wrong == MODEL_ROWS[name] and wrong >= 100
    # falling: for queries 590 .. 592 (whose candidates at min_separation 3 all lie below 590) the first 64 per wave to arrive ARE the best, so
    # that model passes there -- what falling shows is that a newcomer behind all 64 keys must be dropped, for each of the last ten queries
    S, rows = B.score_table("falling"), mirror_rows("falling")
    assert all(wave_model(S, q, 3, 64, "stop") == rows[q] for q in range(590, 593))
    # ... but falling cannot show it: the output is the best 64 of the four lists' 256 keys and never reaches a list's last lane
    assert all(wave_model(S, q, 3, 64, "never") == rows[q] for q in range(590, 600))
    # lone_wave can: the best 64 of queries 590 .. 592 are the list of wave 1 alone, which has met 147 or 148 candidates
    S, rows = B.score_table("lone_wave"), mirror_rows("lone_wave")
    for q in range(590, 593):
        per_wave = [int((S[q, w:q - 2:B.WAVES] > 0).sum()) for w in range(B.WAVES)]
        assert per_wave[1] in (147, 148) and per_wave[0] == per_wave[2] == per_wave[3] == 0, per_wave
        assert wave_model(S, q, 3, 64, "never") != rows[q] and wave_model(S, q, 3, 64, "stop") == rows[q] and len(rows[q]) == 64
    # the model with nothing wrong agrees everywhere: the disagreements above are the steps', not the model's
    for name in B.ALL_VECTOR_SETS:
        S, rows = B.score_table(name), mirror_rows(name)
        assert all(wave_model(S, q, 3, 64, None) == rows[q] for q in range(0, len(S), 7)), name


def test_chain_batch_fills_every_list_and_ties():
    g = B.LOOP
    batch = B.loop_batch()
    assert len(batch) == 320 and all(len(d) == 24 for d in batch) and g["pool"] == 8
    cen, ch = M.train(np.concatenate(batch), g["k"], g["depth"])
    words = [M.descend(cen, ch, d) for d in batch]
    vec = [M.vector(w, M.weights(words, len(ch))) for w in words]
    q = len(vec) - 1
    per_wave = [sum(1 for c in range(w, q - g["min_separation"] + 1, B.WAVES) if M.score(vec[q], vec[c]) > 0) for w in range(B.WAVES)]
    print("chain: candidates with S > 0 per wave for the last query:", per_wave)
    assert min(per_wave) >= 65
    cand, sc = M.shortlist(vec, g["min_separation"], g["T"])
    assert sum(1 for row in sc if len(set(row[row > 0].tolist())) < int((row > 0).sum())) >= 100
