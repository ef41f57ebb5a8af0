"""Binary vocabulary that shortlists loop candidates on the device (binding of include/rgbid_bow.h): a k-majority tree
over the 256-bit descriptors of rgbid.loopfeat, trained on the device, the IDF-weighted bag-of-words vector of a keyframe, the L1 score of
two vectors in integers, and the T best earlier keyframes of every keyframe.

    voc = Vocabulary(ctx, k=10, depth=4)
    voc.train(feats)                                  # or load(ctx, "voc.npz")
    bow = voc.transform(feats)
    cand, scores = voc.shortlist(bow, min_separation=3, T=8)
    pairs, scores = loopfeat.propose(lf, feats, shortlist=voc)"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, ci, vp

ENTRY_DTYPE = np.dtype([("word", "<u4"), ("value", "<u4")])
assert ENTRY_DTYPE.itemsize == 8
MAX_K, MAX_DEPTH, MAX_LEAVES, MAX_ITERS, MAX_SHORTLIST = 16, 6, 1 << 20, 64, 64
MAX_WEIGHT = 726816            # RGBID_BOW_MAX_WEIGHT: the largest weight training can produce; import_ refuses a larger one
ONE = 1 << 30                  # what the values of a vector sum to (at most)
SIGNATURES = {
    "rgbid_bow_create": (vp, vp, ci, ci),
    "rgbid_bow_destroy": (vp,),
    "rgbid_bow_max_nodes": (ci, ci, vp),
    "rgbid_bow_train": (vp, vp, vp, ci, ci, ci),
    "rgbid_bow_set_weights": (vp, vp, vp, ci, ci),
    "rgbid_bow_export": (vp, vp, vp, vp, vp),
    "rgbid_bow_import": (vp, ci, vp, vp, vp),
    "rgbid_bow_transform": (vp, vp, vp, ci, ci, vp, vp, vp),
    "rgbid_bow_score": (vp, vp, vp, ci, ci, vp, ci, vp),
    "rgbid_bow_shortlist": (vp, vp, vp, ci, ci, ci, ci, vp, vp),
    "rgbid_bow_timing": (vp, ci, vp),
}
EXPORTS = list(SIGNATURES)
STAGES = ("train", "transform", "score", "shortlist")


def max_nodes(k, depth):
    """rgbid_bow_max_nodes: the nodes a full tree has; RgbidError outside the limits.  Needs no device."""
    n = C.c_int32(0)
    check(_lib.bind(SIGNATURES).rgbid_bow_max_nodes(int(k), int(depth), C.byref(n)))
    return int(n.value)


class Bow:
    """entries [n, max_keypoints, 2] int32 (word, value; the bits of uint32) and counts [n] int32 on the device; words [n, max_keypoints]
    int32 (the word of each descriptor, -1 in unused slots) when the transform was asked for them, else None"""

    def __init__(self, entries, counts, words=None):
        self.entries, self.counts, self.words = entries, counts, words

    def __len__(self):
        return int(self.entries.shape[0])

    def numpy(self):
        """-> (structured ENTRY_DTYPE [n, max_keypoints], counts [n])"""
        e = self.entries.cpu().numpy()
        return e.view(ENTRY_DTYPE).reshape(e.shape[0], e.shape[1]), self.counts.cpu().numpy()


class Vocabulary(_lib.CtxHandle):
    """A vocabulary tree of branching factor k and depth `depth` on the context's stream; untrained it is the root alone."""
    _destroy, _signatures, _timing, _stages = "rgbid_bow_destroy", SIGNATURES, "rgbid_bow_timing", STAGES

    def __init__(self, ctx, k=10, depth=4):
        super().__init__(ctx)
        self.k, self.depth = int(k), int(depth)
        self._created(self.L.rgbid_bow_create(C.byref(self._h), ctx._h, self.k, self.depth))
        self.dev = self._dev

    @staticmethod
    def _feat_args(feats):
        n = len(feats)
        return (feats.kps.data_ptr() if n else None, feats.counts.data_ptr() if n else None, n, int(feats.kps.shape[1]))

    def train(self, feats, iters=10):
        """train on the descriptors of `feats` (loopfeat.Features) in (keyframe, slot) order and set the weights from them.  Synchronises."""
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_bow_train(self._h, *self._feat_args(feats), int(iters)))
        self.ctx.sync()
        return self

    def set_weights(self, feats):
        """the weights from another set of keyframes.  Synchronises."""
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_bow_set_weights(self._h, *self._feat_args(feats)))
        self.ctx.sync()
        return self

    def export(self):
        """-> dict(k, depth, centroids uint8 [nodes, 32], children int32 [nodes, 2] = first child, number of children, weights uint32 [nodes])"""
        n = C.c_int32(0)
        check(self.L.rgbid_bow_export(self._h, C.byref(n), None, None, None))
        cen = np.zeros((n.value, 32), np.uint8); ch = np.zeros((n.value, 2), np.int32); w = np.zeros(n.value, np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(self.L.rgbid_bow_export(self._h, C.byref(n), p(cen), p(ch), p(w)))
        return dict(k=self.k, depth=self.depth, centroids=cen, children=ch, weights=w)

    def import_(self, centroids, children, weights):
        """the reverse of export; RgbidError for a tree that is not numbered as include/rgbid_bow.h says, does not fit k and depth or holds a
        weight above MAX_WEIGHT"""
        cen = np.ascontiguousarray(centroids, np.uint8).reshape(-1, 32)
        ch = np.ascontiguousarray(children, np.int32).reshape(-1, 2)
        w = np.ascontiguousarray(weights, np.uint32).reshape(-1)
        if not len(cen) == len(ch) == len(w):
            raise ValueError(f"centroids, children and weights disagree on the number of nodes: {len(cen)}, {len(ch)}, {len(w)}")
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(self.L.rgbid_bow_import(self._h, len(cen), p(cen), p(ch), p(w)))
        return self

    def save(self, path):
        """one .npz: k, depth, centroids, children, weights"""
        with open(path, "wb") as f:
            np.savez(f, **self.export())

    def transform(self, feats, words=False):
        """-> Bow of the keyframes of `feats` (with the word of every descriptor when words is set).  Synchronises."""
        kp, cnt, n, mk = self._feat_args(feats)
        ent = torch.zeros((n, mk, 2), dtype=torch.int32, device=self.dev)
        counts = torch.zeros((n,), dtype=torch.int32, device=self.dev)
        wd = torch.full((n, mk), -1, dtype=torch.int32, device=self.dev) if words else None
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_bow_transform(self._h, kp, cnt, n, mk, wd.data_ptr() if (words and n) else None, ent.data_ptr() if n else None,
                                         counts.data_ptr() if n else None))
        self.ctx.sync()
        return Bow(ent, counts, wd)

    def score(self, bow, pairs):
        """S(q, c) of pairs [(q, c)] -> uint64 [P] (numpy).  Synchronises."""
        p = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        P, n = len(p), len(bow)
        pd = torch.from_numpy(p).to(self.dev)
        out = torch.zeros((P,), dtype=torch.int64, device=self.dev)
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_bow_score(self._h, bow.entries.data_ptr() if n else None, bow.counts.data_ptr() if n else None, n,
                                     int(bow.entries.shape[1]), pd.data_ptr() if P else None, P, out.data_ptr() if P else None))
        self.ctx.sync()
        return out.cpu().numpy().view(np.uint64)

    def shortlist(self, bow, min_separation=3, T=8):
        """-> (candidates int32 [n, T], -1 padded; scores uint64 [n, T]) as numpy arrays: per keyframe q the T best c <= q - min_separation
        of score > 0 by (score descending, c descending).  Synchronises."""
        n, T = len(bow), int(T)
        cand = torch.full((n, max(T, 0)), -1, dtype=torch.int32, device=self.dev)
        sc = torch.zeros((n, max(T, 0)), dtype=torch.int64, device=self.dev)
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_bow_shortlist(self._h, bow.entries.data_ptr() if n else None, bow.counts.data_ptr() if n else None, n,
                                         int(bow.entries.shape[1]), int(min_separation), T, cand.data_ptr() if n else None,
                                         sc.data_ptr() if n else None))
        self.ctx.sync()
        return cand.cpu().numpy(), sc.cpu().numpy().view(np.uint64)


def load(ctx, path):
    """a Vocabulary from the .npz that Vocabulary.save wrote"""
    with np.load(path) as z:
        voc = Vocabulary(ctx, int(z["k"]), int(z["depth"]))
        try:
            return voc.import_(z["centroids"], z["children"], z["weights"])
        except Exception:
            voc.close()
            raise


def shortlist_pairs(cand):
    """the pair list the shortlisted proposal matches: per keyframe q >= 1 the pair (q, q - 1) for the normalisation, then (q, c) over its
    candidate row in order"""
    out = []
    for q in range(1, len(cand)):
        out.append((q, q - 1))
        out += [(q, int(c)) for c in cand[q] if c >= 0]
    return out
