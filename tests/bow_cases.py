"""The inputs the binary vocabulary (include/rgbid_bow.h, csrc/kernels_bow.hip) is held to tests/bow_mirror.py on, chosen by the paths of the
kernels and not by convenience.  Plain numpy and the mirror; torch and the package are imported only by the two upload functions (feats_of,
bow_of), so tests/test_cpu_bow_cases.py can assert on the CPU the properties that make each case mean something.  Every seed is in a table.

 training   TRAIN_SHAPES: trees whose split levels hold more than 256 nodes, so that k_bow_finish_scan's threads sum runs of per =
            ceil(N / 256) >= 2 nodes (N = 622: per 3, 208 busy threads, the last run short; 1 000: per 4, 250 busy; 1 024: per 4, all busy; 4 096:
            per 16) and k_bow_seed_set / k_bow_finish_rows get further blocks of nodes and rows.  ITERS_SHAPE at ITERS: the Lloyd passes cut off
            before they converge, and left to run far past it.  ragged_batch: keyframes shorter than the 64-slot vote chunk, a fifteenth of them
            empty.
 transform  transform_batch: keyframe sizes around every power of two of the bitonic sort and every 256-wide chunk of the run-head
            compaction; 1 536 descriptors in 1 536 words; one word 1 536 times; two words whose first run lies across the chunk edge at 256.
            extreme_vocabulary: the largest weight training can produce next to the smallest, which gives an entry of value 0.
 vectors    hand-made bag-of-words vectors for score and shortlist: `rising`, `falling`, `ties`, `sparse` (see each function), 600 keyframes
            of at most 16 entries, so that each of the shortlist's four waves meets far more than the 64 candidates its list holds;
            `lone_wave`, in which one wave's list alone is the answer.
            loop_batch: 320 small keyframes from a pool of 8 for the chain train -> transform -> shortlist."""
import functools

import numpy as np

from tests import bow_mirror as M

MAXKP = 1000
ONE = 1 << 30
MAX_WEIGHT = 726816            # floor(ln(65535) * 65536 + 0.5): the largest weight training can produce (N = 65 535 keyframes, n_w = 1)
BT, VCHUNK, WAVES, LANES = 256, 64, 4, 64      # threads of a block, slots a vote block walks, waves of a shortlist block, keys a wave keeps


# ---- generators ----
def uniform(r, n):
    return r.integers(0, 256, (n, 32), dtype=np.uint8)


def clustered(r, n, prototypes=50, flip=0.1):
    """n descriptors around `prototypes` random ones, each bit flipped with probability `flip`"""
    proto = np.unpackbits(uniform(r, prototypes), axis=1, bitorder="little")
    b = proto[r.integers(0, prototypes, n)] ^ (r.random((n, 256)) < flip).astype(np.uint8)
    return np.packbits(b, axis=1, bitorder="little")


def chunks(desc, size=MAXKP):
    return [desc[s:s + size] for s in range(0, len(desc), size)]


def feats_of(per_kf, max_kp=MAXKP, seed=1, counts=None):
    """descriptor arrays [c_i, 32] per keyframe -> loopfeat.Features; the unused slots hold random descriptors that nothing may read.
    `counts` overrides the counts the device is given (the descriptors stay where they are)."""
    import torch
    from rgbid import loopfeat as LF
    r = np.random.default_rng(seed)
    n = len(per_kf)
    kp = np.zeros((n, max_kp), LF.KP_DTYPE)
    kp["desc"] = r.integers(0, 256, (n, max_kp, 32), dtype=np.uint8)
    cnt = np.zeros(n, np.int32)
    for i, d in enumerate(per_kf):
        kp["desc"][i, :len(d)] = d
        cnt[i] = len(d)
    if counts is not None:
        cnt = np.asarray(counts, np.int32).reshape(n)
    raw = np.ascontiguousarray(kp).view(np.uint8).reshape(n, max_kp, 120)
    return LF.Features(torch.from_numpy(raw).cuda(), torch.from_numpy(cnt).cuda())


# ---- training ----
# (k, depth, n, kind, seed): the nodes per level of the mirror's tree are in tests/test_cpu_bow_cases.py (LEVELS), asserted exactly
TRAIN_SHAPES = (
    (10, 4, 6000, "uniform", 20261020),
    (10, 4, 6000, "clustered", 1004),
    (4, 6, 6000, "uniform", 165),
    (16, 4, 12000, "uniform", 1234),
    (10, 4, 2571, "uniform", 149),
)
DEFAULT_SHAPE = TRAIN_SHAPES[0]
ITERS_SHAPE = (10, 2, 3000, "uniform", 10020)
ITERS = (1, 2, 64)
RAGGED = dict(n_kf=300, max_kp=37, empty=20, k=10, depth=4, seed=3737)


@functools.lru_cache(maxsize=None)
def descriptors(n, kind, seed):
    d = (uniform if kind == "uniform" else clustered)(np.random.default_rng(seed), n)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def mirror_tree(k, depth, n, kind, seed, iters=10):
    """the mirror's (centroids, children) of a training shape, computed once and shared"""
    cen, ch = M.train(descriptors(n, kind, seed), k, depth, iters)
    cen.setflags(write=False); ch.setflags(write=False)
    return cen, ch


def level_sizes(children):
    """nodes per level of a tree in the contract's numbering"""
    sizes, start, end = [], 0, 1
    while start < end:
        sizes.append(end - start)
        start, end = end, end + int(children[start:end, 1].sum())
    return sizes


def split_levels(children):
    """-> the sizes of the levels that hold at least one node with children: the N k_bow_finish_scan meets with something to number"""
    out, start, end = [], 0, 1
    while start < end:
        kids = int(children[start:end, 1].sum())
        if kids:
            out.append(end - start)
        start, end = end, end + kids
    return out


@functools.lru_cache(maxsize=None)
def ragged_batch():
    """-> list of descriptor arrays: RAGGED['n_kf'] keyframes of 0 .. max_kp uniform descriptors, at least RAGGED['empty'] of them empty"""
    g = RAGGED
    r = np.random.default_rng(g["seed"])
    counts = r.integers(0, g["max_kp"] + 1, g["n_kf"])
    counts[r.choice(g["n_kf"], g["empty"], replace=False)] = 0
    desc = uniform(r, int(counts.sum()))
    cuts = np.concatenate([[0], np.cumsum(counts)])
    return [desc[cuts[i]:cuts[i + 1]] for i in range(g["n_kf"])]


def chunk_census(counts, max_kp, chunk=VCHUNK):
    """per vote chunk of `chunk` consecutive slots of the [n_kf][max_kp] layout: (keyframes with a used slot in it, unused slots in it)"""
    used = (np.arange(max_kp)[None, :] < np.asarray(counts)[:, None]).reshape(-1)
    kf = np.repeat(np.arange(len(counts)), max_kp)
    out = []
    for s in range(0, len(used), chunk):
        u = used[s:s + chunk]
        out.append((len(np.unique(kf[s:s + chunk][u])), int((~u).sum())))
    return out


# ---- transform ----
TRANSFORM_COUNTS = (1, 2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535, 1536)
TRANSFORM_SEED = 777
TRANSFORM_MAXKP = 1536
WEIGHT_SET = dict(n_kf=24, seed=778)
TWO_WORD_RUN = 300


@functools.lru_cache(maxsize=None)
def weight_set():
    """the keyframes the transform vocabulary takes its weights from: the training descriptors of DEFAULT_SHAPE, those of a word together in
    1 .. 5 consecutive ones of 24 keyframes, so that the words take five different weights and none is in every keyframe"""
    desc = descriptors(*DEFAULT_SHAPE[2:])
    cen, ch = mirror_tree(*DEFAULT_SHAPE)
    words = M.descend(cen, ch, desc)
    g = WEIGHT_SET
    r = np.random.default_rng(g["seed"])
    m = r.integers(1, 6, len(ch))[words]
    first = r.integers(0, g["n_kf"], len(ch))[words]
    return [desc[(j - first) % g["n_kf"] < m] for j in range(g["n_kf"])]


@functools.lru_cache(maxsize=None)
def transform_batch():
    """-> (keyframes, names): one keyframe per count of TRANSFORM_COUNTS drawn from the training descriptors of DEFAULT_SHAPE, then `distinct`
    (1 536 descriptors in 1 536 words), `copies` (one descriptor 1 536 times) and `two_words` (300 + 300 descriptors of two words, interleaved
    in the input; sorted, the lower word's run spans 0 .. 299)"""
    k, depth, n, kind, seed = DEFAULT_SHAPE
    desc = descriptors(n, kind, seed)
    cen, ch = mirror_tree(*DEFAULT_SHAPE)
    r = np.random.default_rng(TRANSFORM_SEED)
    kfs = [desc[r.choice(n, c, replace=False)] for c in TRANSFORM_COUNTS]
    names = [f"count {c}" for c in TRANSFORM_COUNTS]
    words = M.descend(cen, ch, desc)
    _, one_per_leaf = np.unique(words, return_index=True)
    pick = r.permutation(one_per_leaf)[:TRANSFORM_MAXKP]            # in no order: the sort has work to do
    kfs.append(desc[pick]); names.append("distinct")
    kfs.append(np.tile(desc[int(pick[0])], (TRANSFORM_MAXKP, 1))); names.append("copies")
    lo, hi = sorted((int(pick[1]), int(pick[2])), key=lambda i: words[i])
    two = np.empty((2 * TWO_WORD_RUN, 32), np.uint8)
    two[0::2], two[1::2] = desc[hi], desc[lo]                       # the higher word first
    kfs.append(two); names.append("two_words")
    return kfs, names


EXTREME_PAIRS = ((0, 7), (1535, 1), (1, 1535), (1536, 0), (768, 768))      # descriptors of the heavy word, of the light word
EXTREME_SEED = 779


@functools.lru_cache(maxsize=None)
def extreme_vocabulary(heavy=MAX_WEIGHT, light=1):
    """-> (centroids, children, weights, keyframes): a (2, 1) tree built by hand whose leaves weigh `heavy` and `light`, and keyframes of the two
    centroids themselves in the numbers of EXTREME_PAIRS.  Keyframe 0 holds the light word alone."""
    r = np.random.default_rng(EXTREME_SEED)
    c = uniform(r, 2)
    cen = np.concatenate([np.zeros((1, 32), np.uint8), c])
    ch = np.array([[1, 2], [0, 0], [0, 0]], np.int32)
    W = np.array([0, heavy, light], np.uint32)
    kfs = []
    for nh, nl in EXTREME_PAIRS:
        d = np.concatenate([np.tile(c[0], (nh, 1)), np.tile(c[1], (nl, 1))])
        kfs.append(d[r.permutation(len(d))])
    return cen, ch, W, kfs


# ---- hand-made vectors ----
VEC_N, VEC_MAXKP = 600, 16
VEC_STEP = 1000
SHORTLIST_SETTINGS = ((1, 64), (3, 64), (3, 8), (3, 1), (598, 8), (600, 8))       # (min_separation, T)
VECTOR_SETS = ("rising", "falling", "ties", "sparse")
ALL_VECTOR_SETS = VECTOR_SETS + ("lone_wave",)
VECTOR_SEEDS = dict(ties=881, sparse=882)
# five sets of four words, any two of which share exactly one (the ten edges of the complete graph on five vertices)
TIE_WORDS = ((0, 1, 2, 3), (0, 4, 5, 6), (1, 4, 7, 8), (2, 5, 7, 9), (3, 6, 8, 9))
SPARSE_WORDS = 200


def rising(n=VEC_N):
    """keyframe c = [(0, (c + 1) 1000), (1, ONE - (c + 1) 1000)]: S(q, c) = ONE - 1000 (q - c) grows with c, so every candidate a wave meets is
    its best so far, enters the list at lane 0, and, the list full, pushes the last lane's key off"""
    return [[(0, (c + 1) * VEC_STEP), (1, ONE - (c + 1) * VEC_STEP)] for c in range(n)]


def falling(n=VEC_N, last=10):
    """keyframes below n - 10 = [(0, (n - c) 1000), (1, ONE - (n - c) 1000)], the last ten = [(0, ONE)]: for those ten queries S(q, c) =
    (n - c) 1000 falls with c, so once a wave's list is full every newcomer ranks behind all 64 keys (pos == 64) and is dropped"""
    return [[(0, (n - c) * VEC_STEP), (1, ONE - (n - c) * VEC_STEP)] if c < n - last else [(0, ONE)] for c in range(n)]


def lone_wave(n=VEC_N, last=10, wave=1):
    """`falling` with every keyframe below n - 10 emptied but those of one wave (c % 4 == 1).  In `falling` a wave's last lane never reaches
    the output, which takes the best 64 of the four lists' 256 keys; here the best 64 of queries 590 .. 592 ARE one wave's list, so a newcomer
    that took the last lane instead of being dropped would show"""
    return [v if c >= n - last or c % WAVES == wave else [] for c, v in enumerate(falling(n, last))]


def ties(n=VEC_N):
    """each keyframe one of the five vectors of TIE_WORDS with four values of ONE // 4, one in ten empty: S is ONE, ONE // 4 or 0, and hundreds
    of equal scores are ordered by c alone"""
    r = np.random.default_rng(VECTOR_SEEDS["ties"])
    pick = r.integers(0, len(TIE_WORDS), n)
    return [[] if c % 10 == 0 else [(w, ONE // 4) for w in TIE_WORDS[pick[c]]] for c in range(n)]


def sparse(n=VEC_N):
    """random vectors of 1 .. 16 of 200 words (word w drawn with probability ~ 1 / (w + 8), values that sum to ONE); one keyframe in five
    (c % 5 == 2) takes its words from a range no one else uses and scores 0 against everyone; one in ten (c % 10 == 0) is empty.  The last
    keyframe holds 16 words."""
    r = np.random.default_rng(VECTOR_SEEDS["sparse"])
    p = 1.0 / (np.arange(SPARSE_WORDS) + 8.0)
    p /= p.sum()
    out = []
    for c in range(n):
        m = VEC_MAXKP if c == n - 1 else int(r.integers(1, VEC_MAXKP + 1))
        words = np.sort(r.choice(SPARSE_WORDS, m, replace=False, p=p))
        cuts = np.sort(r.integers(0, ONE + 1, m - 1))
        vals = np.diff(np.concatenate([[0], cuts, [ONE]]))
        if c % 10 == 0:
            out.append([])
        elif c % 5 == 2:
            out.append([(1000 + VEC_MAXKP * c + j, int(v)) for j, v in enumerate(vals)])
        else:
            out.append([(int(w), int(v)) for w, v in zip(words, vals)])
    return out


@functools.lru_cache(maxsize=None)
def vector_set(name):
    return tuple(tuple(v) for v in {"rising": rising, "falling": falling, "ties": ties, "sparse": sparse, "lone_wave": lone_wave}[name]())


@functools.lru_cache(maxsize=None)
def score_table(name):
    """S(q, c) of a vector set by the mirror for all c < q -> int64 [n, n] (0 elsewhere), computed once and shared"""
    v = vector_set(name)
    n = len(v)
    S = np.zeros((n, n), np.int64)
    for q in range(n):
        for c in range(q):
            S[q, c] = M.score(v[q], v[c])
    S.setflags(write=False)
    return S


def pack_vectors(vectors, max_kp=VEC_MAXKP):
    """-> (entries int32 [n, max_kp, 2] holding the bits of (word, value) uint32, counts int32 [n])"""
    n = len(vectors)
    ent = np.zeros((n, max_kp, 2), np.uint32)
    cnt = np.zeros(n, np.int32)
    for i, v in enumerate(vectors):
        assert len(v) <= max_kp and all(a[0] < b[0] for a, b in zip(v, v[1:])) and sum(x for _, x in v) <= ONE
        cnt[i] = len(v)
        if len(v):
            ent[i, :len(v)] = np.array(v, np.uint32)
    return ent.view(np.int32), cnt


def bow_of(vectors, max_kp=VEC_MAXKP):
    """hand-made vectors -> rgbid.bow.Bow on the device"""
    import torch
    from rgbid import bow as BW
    ent, cnt = pack_vectors(vectors, max_kp)
    return BW.Bow(torch.from_numpy(ent).cuda(), torch.from_numpy(cnt).cuda())


# ---- the chain on many small keyframes ----
LOOP = dict(n_kf=320, per_kf=24, pool=8, k=10, depth=2, seed=883, min_separation=3, T=64)


@functools.lru_cache(maxsize=None)
def loop_batch():
    """320 keyframes of 24 clustered descriptors, each one of a pool of 8 sets, so that equal keyframes tie exactly"""
    g = LOOP
    r = np.random.default_rng(g["seed"])
    pool = [clustered(r, g["per_kf"]) for _ in range(g["pool"])]
    return [pool[i] for i in r.integers(0, g["pool"], g["n_kf"])]
