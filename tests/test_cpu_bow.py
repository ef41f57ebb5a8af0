"""CPU checks of the binary vocabulary (include/rgbid_bow.h, rgbid.bow): the numpy restatement the GPU tests compare the kernels against
(tests/bow_mirror.py) on trees worked out by hand; the score identity in integers; the host side of the shortlisted proposal; the header as
C99; the library's exports; refusals that need no device.  (rgbid_bow_import / rgbid_bow_export need a context, whose creation needs a
device: their round trip is in tests/test_gpu_bow.py.)"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from rgbid import _lib
from rgbid import bow as BW
from tests import bow_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def desc(*bits):
    d = np.zeros(32, np.uint8)
    for b in bits:
        d[b // 8] |= 1 << (b % 8)
    return d


def test_three_descriptors_k2_by_hand():
    """A = 0, B = bits 0-3, C = bit 0.  Seeds: A, then B (distance 4 against C's 1).  assign: A -> 0, B -> 1, C -> 0 (1 against 3).  update:
    child 0 holds A and C, bit 0 is set in 1 of 2: a tie clears it, the centroid is 0; child 1 is B.  The next assignment is the same."""
    A, B, C = desc(), desc(0, 1, 2, 3), desc(0)
    cen, ch = M.train(np.stack([A, B, C]), 2, 1)
    assert ch.tolist() == [[1, 2], [0, 0], [0, 0]]
    assert np.array_equal(cen, np.stack([desc(), desc(), B]))
    assert M.descend(cen, ch, np.stack([A, B, C, desc(0, 1)])).tolist() == [1, 2, 1, 1]      # bits 0, 1: distance 2 to both, the lower child
    # depth 2: child 0 (A, C) splits again: seeds A, C; child 1 holds one descriptor and stays a leaf
    cen, ch = M.train(np.stack([A, B, C]), 2, 2)
    assert ch.tolist() == [[1, 2], [3, 2], [0, 0], [0, 0], [0, 0]]
    assert np.array_equal(cen[3], A) and np.array_equal(cen[4], C)


def test_equal_descriptors_and_small_sets():
    """all descriptors equal: the largest distance after the first seed is 0, one seed, the root stays a leaf; n = 0 and n = 1 likewise; n < k
    gives n children"""
    for n in (0, 1, 5):
        cen, ch = M.train(np.tile(desc(3, 77), (n, 1)), 4, 3)
        assert ch.tolist() == [[0, 0]] and not cen.any()
    cen, ch = M.train(np.stack([desc(1), desc(2, 3), desc(1)]), 10, 1)
    assert ch.tolist() == [[1, 2], [0, 0], [0, 0]] and np.array_equal(cen[1], desc(1)) and np.array_equal(cen[2], desc(2, 3))
    # two distinct descriptors repeated: two children however large k is
    cen, ch = M.train(np.stack([desc(1), desc(9)] * 6), 16, 2)
    assert ch.tolist() == [[1, 2], [0, 0], [0, 0]]      # each child holds equal descriptors: no further split


def test_majority_tie_clears_the_bit():
    """child 0 holds 0 and bit 0 (tie: cleared) or 0, bit 0, bit 0 (2 of 3: set); the far seed is 64 bits away"""
    far = desc(*range(8, 72))
    cen, _ = M.train(np.stack([desc(), desc(0), far]), 2, 1)
    assert np.array_equal(cen[1], desc()) and np.array_equal(cen[2], far)
    cen, _ = M.train(np.stack([desc(), desc(0), far, desc(0)]), 2, 1)
    assert np.array_equal(cen[1], desc(0))


def test_farthest_point_tie_takes_the_lowest_index():
    """P = bits 0, 1 and Q = bits 2, 3 are both 2 from the first seed: P (the lower index) is seed 1; with k = 3 Q follows (its minimum is 2,
    everything else 0)"""
    S, P, Q = desc(), desc(0, 1), desc(2, 3)
    cen, ch = M.train(np.stack([S, P, Q]), 2, 1, iters=1)
    assert ch[0].tolist() == [1, 2]
    # seeds S, P; Q is 2 from S and 4 from P: child 0; update: child 0 = {S, Q}: ties clear: 0
    assert np.array_equal(cen[1], S) and np.array_equal(cen[2], P)
    cen, ch = M.train(np.stack([S, P, Q]), 3, 1)
    assert ch[0].tolist() == [1, 3] and np.array_equal(cen[2], P) and np.array_equal(cen[3], Q)
    cen, ch = M.train(np.stack([S, Q, P]), 2, 1)
    assert np.array_equal(cen[2], Q)


def test_weights_and_vector_by_hand():
    """N = 4 keyframes, word 1 in 2 of them, word 2 in all, word 3 in 1: W = round(ln 2 * 65536), 0, round(ln 4 * 65536); a vector of
    counts (2, 5, 1) normalises to a sum within the entries' count of 2^30"""
    W = M.weights([np.array([1, 2]), np.array([2, 2, 1]), np.array([2, 3]), np.array([2])], 5)
    assert W.tolist() == [0, 45426, 0, 90852, 0]
    v = M.vector([1, 1, 2, 2, 2, 2, 2, 3], W)
    A = 2 * 45426 + 90852
    assert v == [(1, ((2 * 45426) << 30) // A), (2, 0), (3, (90852 << 30) // A)]      # the entry of value 0 stays
    assert v[0][1] == v[2][1] == 1 << 29
    assert M.vector([2, 2], W) == [] and M.vector([], W) == []
    assert M.weights([], 3).tolist() == [0, 0, 0]


def test_score_is_the_l1_score_in_integers():
    """for vectors that sum exactly to 2^30, sum of min = 2^30 - (sum |v - w|) / 2 over the union of the words, in integers"""
    r = np.random.default_rng(11)
    for _ in range(50):
        vs = []
        for _ in range(2):
            words = np.sort(r.choice(60, r.integers(1, 40), replace=False))
            cuts = np.sort(r.integers(0, BW.ONE + 1, len(words) - 1))
            vals = np.diff(np.concatenate([[0], cuts, [BW.ONE]]))
            assert vals.sum() == BW.ONE
            vs.append([(int(w), int(v)) for w, v in zip(words, vals)])
        dq, dc = dict(vs[0]), dict(vs[1])
        l1 = sum(abs(dq.get(w, 0) - dc.get(w, 0)) for w in set(dq) | set(dc))
        assert l1 % 2 == 0 and M.score(vs[0], vs[1]) == BW.ONE - l1 // 2
        assert M.score(vs[0], vs[1]) == M.score(vs[1], vs[0])


def test_shortlist_order_and_pairs():
    """equal scores: the later keyframe first; score 0 is no candidate; T cuts; the pair list of the shortlisted proposal"""
    a, b, z = [(1, 600), (2, 400)], [(1, 600), (5, 400)], [(9, 1000)]
    cand, sc = M.shortlist([a, b, z, b, a], 1, 3)
    assert cand.tolist() == [[-1, -1, -1], [0, -1, -1], [-1, -1, -1], [1, 0, -1], [0, 3, 1]]      # 4: 1000 with 0; 600 with 3 and with 1
    assert sc[4].tolist() == [1000, 600, 600] and sc[3].tolist() == [1000, 600, 0]
    assert M.shortlist([a, b, z, b, a], 1, 2)[0][4].tolist() == [0, 3]
    cand, _ = M.shortlist([a, b, z, b, a], 3, 8)
    assert cand[4].tolist()[:3] == [0, 1, -1] and cand[3].tolist()[:2] == [0, -1]
    assert BW.shortlist_pairs(cand[:, :2]) == [(1, 0), (2, 1), (3, 2), (3, 0), (4, 3), (4, 0), (4, 1)]


def test_refusals_without_device():
    assert BW.max_nodes(10, 4) == 11111 and BW.max_nodes(2, 6) == 127 and BW.max_nodes(16, 5) == 1118481
    for bad in ((1, 3), (17, 1), (2, 0), (2, 7), (16, 6), (11, 6)):
        with pytest.raises(_lib.RgbidError):
            BW.max_nodes(*bad)
    L = _lib_handle()
    h = ctypes.c_void_p()
    L.rgbid_bow_create.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    assert L.rgbid_bow_create(ctypes.byref(h), None, 10, 4) == -1 and not h.value
    assert L.rgbid_bow_create(None, None, 10, 4) == -1
    assert L.rgbid_bow_destroy(None) == 0
    assert L.rgbid_bow_train(None, None, None, 0, 1000, 10) == -1
    assert L.rgbid_bow_transform(None, None, None, 0, 1000, None, None, None) == -1
    assert L.rgbid_bow_shortlist(None, None, None, 0, 1000, 3, 8, None, None) == -1
    assert L.rgbid_bow_timing(None, 0, None) == -1


def test_propose_takes_the_shortlist_option():
    import inspect
    from rgbid import loopfeat as LF
    p = inspect.signature(LF.propose).parameters
    assert p["shortlist"].default is None and p["shortlist_size"].default == 8
    a = inspect.signature(LF.appearance_loops).parameters
    assert a["proposal"].default == "match" and a["vocabulary"].default is None
    with pytest.raises(ValueError):
        LF.appearance_loops(None, [dict(), dict()], None, proposal="dbow")


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_bow.c"
    src.write_text('#include "rgbid_bow.h"\n'
                   "typedef char entry_is_8_bytes[sizeof(rgbid_bow_entry) == 8 ? 1 : -1];\n"
                   "int use(rgbid_bow* v, const rgbid_bow_entry* b, const int32_t* c, int32_t* cand, uint64_t* s) {\n"
                   "  return rgbid_bow_shortlist(v, b, c, 2, 1000, 3, 8, cand, s); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def _lib_handle():
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_library_exports_bow_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_bow.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_bow_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(BW.EXPORTS), set(declared) ^ set(BW.EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing
