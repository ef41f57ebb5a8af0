"""Appearance stage of loop closure on the device (binding of include/rgbid_loopfeat.h): binary features of keyframes,
2-NN Hamming matching with the ratio test, the appearance proposal, and the 3-point RANSAC over 3-D correspondences that starts the dense
verifier (LoopCloser::detectLoopClosures / computeRANSACTrafo3D, src/loop_closer.cpp:193-716).

    lf = LoopFeat(ctx, rows, cols)                             # levels=8, scale=1.2: features over a scale pyramid
    feats = lf.extract(grey [n, rows, cols] uint8, invdepth [n, rows, cols] float32, K)
    pairs, scores = propose(lf, feats)                         # uses no pose
    res = lf.ransac(feats, pairs, *lf.match(feats, pairs))     # qTc_ini, best iteration, inliers, mask per pair

`appearance_loops` strings the stages together for rgbid.posegraph.optimise_run(loops="appearance")."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ci, f32, f64, vp

KP_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("response", "<f4"), ("direction", "<i4"), ("desc", "u1", (32,)), ("X", "<f8", (3,)),
                     ("cov", "<f8", (6,))])
assert KP_DTYPE.itemsize == 120
AUX_DTYPE = np.dtype([("px", "<f4"), ("py", "<f4"), ("lx", "<i2"), ("ly", "<i2"), ("level", "<i4")])
assert AUX_DTYPE.itemsize == 16
MATCH_DTYPE = np.dtype([("query", "<i4"), ("train", "<i4"), ("distance", "<i4"), ("second", "<i4")])
assert MATCH_DTYPE.itemsize == 16

CELL, CELL_MAX, BORDER, DIRECTIONS, TESTS = 32, 64, 16, 32, 256
MAX_KEYPOINTS, MAX_ITERS, MAX_LEVELS = 1536, 4096, 8
SIGNATURES = {
    "rgbid_loopfeat_create": (vp, vp, ci, ci, ci),
    "rgbid_loopfeat_create_levels": (vp, vp, ci, ci, ci, ci, f32),
    "rgbid_loopfeat_destroy": (vp,),
    "rgbid_loopfeat_plan_levels": (ci, ci, ci, ci, f32, vp, vp, vp),
    "rgbid_loopfeat_resize_table": (ci, ci, vp, vp),
    "rgbid_loopfeat_tables": (vp, vp, vp),
    "rgbid_loopfeat_layout": (vp, vp, vp, vp),
    "rgbid_loopfeat_level_layout": (vp, ci, vp, vp, vp, vp, vp, vp),
    "rgbid_loopfeat_extract": (vp, vp, vp, ci, vp, vp, vp),
    "rgbid_loopfeat_extract_levels": (vp, vp, vp, ci, vp, vp, vp, vp),
    "rgbid_loopfeat_pyramid": (vp, vp, ci, ci, vp),
    "rgbid_loopfeat_match": (vp, vp, vp, ci, vp, ci, f32, vp, vp),
    "rgbid_loopfeat_ransac": (vp, vp, ci, vp, ci, vp, vp, vp, ci, f64, vp, vp, vp),
    "rgbid_loopfeat_timing": (vp, ci, vp),
    "rgbid_loopfeat_timing_pyramid": (vp, vp),
}
EXPORTS = list(SIGNATURES)
STAGES = ("response", "select", "describe", "match", "ransac")
LEVELS, SCALE = 8, 1.2         # the reference's FEATURE_EXTRACTOR LEVELS and SCALE; the default here is one level

# the reference's settings (config_data/visodoRGBDconfig.ini, loop_closer.cpp)
MATCH_RATIO = 0.75             # MATCH_SCORE_RATIO_THRESHOLD
SCORE_THRESHOLD = 0.6          # NORMALISED_BOW_SCORE_THRESHOLD
MIN_INLIERS = 10               # MIN_REQUIRED_INLIERS
MIN_HULL_RATIO = 0.05
MAHALANOBIS_TH = 4.11
RANSAC_SEED = 0x34985739
RANSAC_CONFIDENCE, RANSAC_INLIER_RATIO, RANSAC_MIN_POINTS = 0.99, 0.3, 3


def num_iters(confidence=RANSAC_CONFIDENCE, inlier_ratio=RANSAC_INLIER_RATIO, points=RANSAC_MIN_POINTS):
    """loop_closer.cpp:386 in float32, as its 1.f and std::pow(float, float) evaluate it: (int)(log(1 - conf) / log(1 - ratio^points) - 1) + 1.
    168 for the reference's settings."""
    f = np.float32
    c, r = f(confidence), f(inlier_ratio)
    v = np.log(f(1.0) - c) / np.log(f(1.0) - np.power(r, f(points), dtype=np.float32)) - f(1.0)
    return int(f(v)) + 1


def uniform_draws(iters, seed=RANSAC_SEED):
    """3 * iters values of Sampler::rand_uniform01 (sampler.cpp:46-51) after prng.reset(seed): MT19937 seeded by init_genrand, as boost::mt19937
    and numpy's RandomState(seed) both are; u = x / 2^32"""
    rs = np.random.RandomState(int(seed))
    return mt19937_words(rs, 3 * int(iters)).astype(np.float64) / (float(0xFFFFFFFF) + 1.0)


def mt19937_words(rs, n):
    """the next n raw 32-bit outputs of a numpy RandomState"""
    return np.frombuffer(rs.bytes(4 * int(n)), dtype="<u4").copy()


def tables():
    """the library's host tables -> (pattern int8 [256, 4], rotated int8 [32, 256, 4], bounds float64 [16, 2])"""
    L = _lib.bind(SIGNATURES)
    pat = np.zeros((TESTS, 4), np.int8); rot = np.zeros((DIRECTIONS, TESTS, 4), np.int8); bnd = np.zeros((16, 2), np.float64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    check(L.rgbid_loopfeat_tables(p(pat), p(rot), p(bnd)))
    return pat, rot, bnd


def layout(rows, cols, max_keypoints):
    """(cells_x, cells_y, keypoints kept per cell) of include/rgbid_loopfeat.h; ValueError for the sizes the library refuses"""
    rows, cols, max_keypoints = int(rows), int(cols), int(max_keypoints)
    if rows < 2 * BORDER + 1 or cols < 2 * BORDER + 1 or rows > 8192 or cols > 8192:
        raise ValueError(f"rows, cols must be {2 * BORDER + 1} .. 8192, got {rows} x {cols}")
    cx, cy = (cols + CELL - 1) // CELL, (rows + CELL - 1) // CELL
    if not cx * cy <= max_keypoints <= MAX_KEYPOINTS:
        raise ValueError(f"max_keypoints must be {cx * cy} (one per cell) .. {MAX_KEYPOINTS}, got {max_keypoints}")
    return cx, cy, min(max_keypoints // (cx * cy), CELL_MAX)


def layout_levels(rows, cols, max_keypoints, levels=1, scale=SCALE):
    """the levels of include/rgbid_loopfeat.h that exist -> [(rows_l, cols_l, cells_x, cells_y, per_cell, s_l)]; ValueError for what the
    library refuses (rgbid_loopfeat_plan_levels is the same on the C side)"""
    f32 = np.float32
    rows, cols, max_keypoints, levels, scale = int(rows), int(cols), int(max_keypoints), int(levels), f32(scale)
    if rows < 2 * BORDER + 1 or cols < 2 * BORDER + 1 or rows > 8192 or cols > 8192:
        raise ValueError(f"rows, cols must be {2 * BORDER + 1} .. 8192, got {rows} x {cols}")
    if not 1 <= levels <= MAX_LEVELS or not (scale > f32(1.0) and scale <= f32(2.0)):
        raise ValueError(f"levels must be 1 .. {MAX_LEVELS} and 1 < scale <= 2, got {levels}, {scale}")
    if not 1 <= max_keypoints <= MAX_KEYPOINTS:
        raise ValueError(f"max_keypoints must be 1 .. {MAX_KEYPOINTS}, got {max_keypoints}")
    geo = []
    for l in range(levels):
        s = f32(math.pow(float(scale), float(l)))
        c, r = int((f32(cols) + f32(0.5)) / s), int((f32(rows) + f32(0.5)) / s)
        if r < 2 * BORDER + 1 or c < 2 * BORDER + 1:
            break
        geo.append((r, c, (c + CELL - 1) // CELL, (r + CELL - 1) // CELL, s))
    sd = float(scale)
    r = 1.0 / (sd * sd)
    rL = 1.0
    for _ in geo:
        rL *= r
    out, rl, slots = [], 1.0, 0
    for rows_l, cols_l, cx, cy, s in geo:
        n = int(math.floor(float(max_keypoints) * (((1.0 - r) * rl) / (1.0 - rL))))
        k = min(max(n // (cx * cy), 1), CELL_MAX)
        out.append((rows_l, cols_l, cx, cy, k, float(s)))
        slots += cx * cy * k
        rl *= r
    if slots > max_keypoints:
        raise ValueError(f"{len(out)} levels of {rows} x {cols} need {slots} keypoint slots (one per cell at least), max_keypoints is {max_keypoints}")
    return out


def plan_levels(rows, cols, max_keypoints, levels=1, scale=SCALE):
    """rgbid_loopfeat_plan_levels: the library's own answer to layout_levels, the same tuples; RgbidError for its refusals.  Needs no device."""
    L = _lib.bind(SIGNATURES)
    n = C.c_int32(0)
    geo = np.zeros((MAX_LEVELS, 5), np.int32); s = np.zeros(MAX_LEVELS, np.float32)
    check(L.rgbid_loopfeat_plan_levels(int(rows), int(cols), int(max_keypoints), int(levels), C.c_float(float(scale)), C.byref(n),
                                       geo.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p)))
    return [tuple(int(v) for v in geo[l]) + (float(s[l]),) for l in range(n.value)]


def resize_table(src, dst):
    """rgbid_loopfeat_resize_table -> (x0 int32 [dst], w1 int32 [dst]) of one axis.  Needs no device."""
    L = _lib.bind(SIGNATURES)
    x0 = np.zeros(max(int(dst), 0), np.int32); w1 = np.zeros(max(int(dst), 0), np.int32)
    check(L.rgbid_loopfeat_resize_table(int(src), int(dst), x0.ctypes.data_as(C.c_void_p), w1.ctypes.data_as(C.c_void_p)))
    return x0, w1


class Features:
    """records [n, max_keypoints, 120] uint8 and counts [n] int32 on the device; aux [n, max_keypoints, 16] uint8 (level, level pixel and
    float position of each record) when the extraction was asked for it, else None"""

    def __init__(self, kps, counts, aux=None):
        self.kps, self.counts, self.aux = kps, counts, aux

    def __len__(self):
        return int(self.kps.shape[0])

    def numpy(self):
        """-> (structured KP_DTYPE [n, max_keypoints], counts [n])"""
        return self.kps.cpu().numpy().view(KP_DTYPE).reshape(self.kps.shape[0], self.kps.shape[1]), self.counts.cpu().numpy()

    def numpy_aux(self):
        """-> structured AUX_DTYPE [n, max_keypoints]"""
        if self.aux is None:
            raise ValueError("these features were extracted without aux records (extract(..., aux=True))")
        return self.aux.cpu().numpy().view(AUX_DTYPE).reshape(self.aux.shape[0], self.aux.shape[1])


class LoopFeat(_lib.CtxHandle):
    """Feature extractor, matcher and RANSAC for keyframes of rows x cols pixels, on the context's stream.  levels > 1: features over a
    pyramid of that many images at `scale` between neighbours (self.levels lists those that exist), so that a revisit at another distance
    still matches; levels = 1 is the single-level extractor."""
    _destroy, _signatures, _timing, _stages = "rgbid_loopfeat_destroy", SIGNATURES, "rgbid_loopfeat_timing", STAGES

    def __init__(self, ctx, rows, cols, max_keypoints=1000, levels=1, scale=SCALE):
        super().__init__(ctx)
        self.rows, self.cols, self.max_keypoints = int(rows), int(cols), int(max_keypoints)
        if int(levels) == 1:
            self.cells_x, self.cells_y, self.per_cell = layout(rows, cols, max_keypoints)
        self.levels = layout_levels(rows, cols, max_keypoints, levels, scale)
        _, _, self.cells_x, self.cells_y, self.per_cell, _ = self.levels[0]
        self.scale = float(np.float32(scale))
        self._created(self.L.rgbid_loopfeat_create_levels(C.byref(self._h), ctx._h, self.rows, self.cols, self.max_keypoints, int(levels),
                                                          C.c_float(self.scale)))
        self.dev = self._dev

    def _on_device(self, a, dtype):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(device=self.dev, dtype=dtype).contiguous()

    def timing_pyramid(self):
        """the device ms the last timed extract spent on its pyramid (0.0 with one level)"""
        return self._stage_ms("rgbid_loopfeat_timing_pyramid", ("pyramid",))["pyramid"]

    def level_layout(self, level):
        """rgbid_loopfeat_level_layout -> (rows_l, cols_l, cells_x, cells_y, per_cell, s_l) as the library holds it"""
        v = [C.c_int(0) for _ in range(5)]
        s = C.c_float(0.0)
        check(self.L.rgbid_loopfeat_level_layout(self._h, int(level), *[C.byref(x) for x in v], C.byref(s)))
        return tuple(x.value for x in v) + (float(s.value),)

    def pyramid(self, grey, level):
        """level `level` of the pyramid of grey [n, rows, cols] uint8 -> [n, rows_l, cols_l] uint8 on the device.  Synchronises."""
        g = self._on_device(grey, torch.uint8)
        assert g.dim() == 3 and tuple(g.shape[1:]) == (self.rows, self.cols), g.shape
        if not 0 <= int(level) < len(self.levels):
            raise ValueError(f"level {level} does not exist (levels 0 .. {len(self.levels) - 1})")
        n = int(g.shape[0])
        out = torch.zeros((n, self.levels[level][0], self.levels[level][1]), dtype=torch.uint8, device=self.dev)
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_loopfeat_pyramid(self._h, g.data_ptr() if n else None, n, int(level), out.data_ptr() if n else None))
        self.ctx.sync()
        return out

    def extract(self, grey, invdepth, K, aux=False):
        """grey [n, rows, cols] uint8 and invdepth [n, rows, cols] float32 (numpy or tensors), K = (fx, fy, cx, cy) -> Features (with the
        16-byte aux records when aux is set).  Synchronises."""
        g, w = self._on_device(grey, torch.uint8), self._on_device(invdepth, torch.float32)
        assert g.dim() == 3 and tuple(g.shape[1:]) == (self.rows, self.cols) and g.shape == w.shape, (g.shape, w.shape)
        n = int(g.shape[0])
        kps = torch.empty((n, self.max_keypoints, 120), dtype=torch.uint8, device=self.dev)
        counts = torch.zeros((n,), dtype=torch.int32, device=self.dev)
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        self.ctx.wait_torch_stream()
        ax = torch.empty((n, self.max_keypoints, 16), dtype=torch.uint8, device=self.dev) if aux else None
        check(self.L.rgbid_loopfeat_extract_levels(self._h, g.data_ptr() if n else None, w.data_ptr() if n else None, n, Kc,
                                                   kps.data_ptr() if n else None, counts.data_ptr() if n else None,
                                                   ax.data_ptr() if (aux and n) else None))
        self.ctx.sync()
        return Features(kps, counts, ax)

    def _pairs(self, pairs):
        p = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        return p, self._on_device(p, torch.int32)

    def match(self, feats, pairs, ratio=MATCH_RATIO, lists=True):
        """pairs [(query, candidate)] keyframe indices -> (matches [P, max_keypoints, 16] uint8 on the device (None without lists), counts [P]
        int32 on the device).  Synchronises."""
        p, pd = self._pairs(pairs)
        P = len(p)
        counts = torch.zeros((P,), dtype=torch.int32, device=self.dev)
        m = torch.zeros((P, self.max_keypoints, 16), dtype=torch.uint8, device=self.dev) if lists else None
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_loopfeat_match(self._h, feats.kps.data_ptr() if len(feats) else None, feats.counts.data_ptr() if len(feats) else None,
                                          len(feats), pd.data_ptr() if P else None, P, C.c_float(float(ratio)),
                                          m.data_ptr() if (lists and P) else None, counts.data_ptr() if P else None))
        self.ctx.sync()
        return m, counts

    def ransac(self, feats, pairs, matches, match_counts, iters=None, seed=RANSAC_SEED, threshold=MAHALANOBIS_TH, u=None):
        """-> dict(R [P, 3, 3], t [P, 3], best [P], inliers [P], mask [P, max_keypoints] uint8) as numpy arrays.  u: the 3 * iters uniform
        draws (default: uniform_draws(iters, seed); iters default num_iters()).  Synchronises."""
        p, pd = self._pairs(pairs)
        P = len(p)
        if u is None:
            iters = num_iters() if iters is None else int(iters)
            u = uniform_draws(iters, seed)
        u = np.ascontiguousarray(u, np.float64)
        iters = len(u) // 3
        ud = self._on_device(u, torch.float64)
        pose = torch.zeros((P, 12), dtype=torch.float64, device=self.dev)
        res = torch.zeros((P, 2), dtype=torch.int32, device=self.dev)
        mask = torch.zeros((P, self.max_keypoints), dtype=torch.uint8, device=self.dev)
        self.ctx.wait_torch_stream()
        q = lambda t_: t_.data_ptr() if P else None
        check(self.L.rgbid_loopfeat_ransac(self._h, feats.kps.data_ptr() if len(feats) else None, len(feats), q(pd), P,
                                           matches.data_ptr() if (matches is not None and P) else None, q(match_counts), ud.data_ptr(), iters,
                                           C.c_double(float(threshold)), q(pose), q(res), q(mask)))
        self.ctx.sync()
        po, r = pose.cpu().numpy(), res.cpu().numpy()
        return dict(R=po[:, :9].reshape(-1, 3, 3).copy(), t=po[:, 9:].copy(), best=r[:, 0].copy(), inliers=r[:, 1].copy(), mask=mask.cpu().numpy())


# ---- host side of the proposal and of the gates ----
def all_pairs(n, min_separation=3):
    """every (q, c) the proposal scores: c <= q - min_separation, and (q, q - 1) for the normalisation"""
    out = []
    for q in range(1, n):
        out.append((q, q - 1))
        out += [(q, c) for c in range(0, q - min_separation + 1)]
    return out


def select_candidates(n, counts, min_separation=3, score_threshold=SCORE_THRESHOLD, per_query=(2, 2)):
    """loop_closer.cpp:203-271 with the match count as the appearance score: counts {(q, c): matches}.  For each keyframe q the candidates
    c <= q - min_separation whose count / count(q, q - 1) exceeds the threshold (float32, as the reference divides); of those the
    per_query[0] of largest separation, then the per_query[1] of best score (the later keyframe first on equal scores, as the reference's
    multimap is walked from its end), without duplicates.  -> ([(q, c)], {(q, c): normalised score})"""
    out, scores = [], {}
    for q in range(1, n):
        ref = np.float32(counts.get((q, q - 1), 0))
        if not ref > 0:
            continue
        cands = []
        for c in range(0, q - min_separation + 1):
            s = np.float32(counts.get((q, c), 0)) / ref
            if s > np.float32(score_threshold):
                cands.append((c, float(s)))
        pick = [c for c, _ in sorted(cands, key=lambda x: x[0])[:per_query[0]]]
        for c, _ in sorted(cands, key=lambda x: (-x[1], -x[0]))[:per_query[1]]:
            if c not in pick:
                pick.append(c)
        sc = dict(cands)
        for c in pick:
            out.append((q, c))
            scores[(q, c)] = sc[c]
    return out, scores


def propose(lf, feats, min_separation=3, score_threshold=SCORE_THRESHOLD, per_query=(2, 2), ratio=MATCH_RATIO, shortlist=None, shortlist_size=8,
            details=None):
    """Appearance proposal over the keyframes of `feats` (in order): one matching call over all (q, c) pairs, then select_candidates.
    It uses no pose.  shortlist: a rgbid.bow.Vocabulary; the matching call then runs over (q, q - 1) and the shortlist_size candidates the
    vocabulary ranks best for q instead of over all pairs, and select_candidates sees those counts alone.  details (a dict) receives the
    shortlist: candidates [n, T], bow_scores [n, T].  -> ([(q, c)], {(q, c): normalised score})"""
    n = len(feats)
    if shortlist is None:
        pairs = all_pairs(n, min_separation)
    else:
        from . import bow as BW
        cand, sc = shortlist.shortlist(shortlist.transform(feats), min_separation, shortlist_size)
        if details is not None:
            details.update(candidates=cand, bow_scores=sc)
        pairs = BW.shortlist_pairs(cand)
    if not pairs:
        return [], {}
    _, mc = lf.match(feats, pairs, ratio, lists=False)
    counts = dict(zip(pairs, [int(v) for v in mc.cpu().numpy()]))
    return select_candidates(n, counts, min_separation, score_threshold, per_query)


def hull_area(points):
    """computeConvexHullArea (util_funcs.cpp:256-274) over an own monotone-chain hull: |sum (x_{i+1} - x_i) (y_{i+1} + y_i) / 2|"""
    pts = sorted(set((float(x), float(y)) for x, y in points))
    if len(pts) < 3:
        return 0.0

    def half(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and (h[-1][0] - h[-2][0]) * (p[1] - h[-2][1]) - (h[-1][1] - h[-2][1]) * (p[0] - h[-2][0]) <= 0:
                h.pop()
            h.append(p)
        return h
    lo, up = half(pts), half(pts[::-1])
    ch = lo[:-1] + up[:-1]
    area = 0.0
    for i in range(len(ch)):
        a, b = ch[i], ch[(i + 1) % len(ch)]
        area += (b[0] - a[0]) * ((b[1] + a[1]) / 2.0)
    return abs(area)


def gate(kq, kc, matches, mask, rows, cols, min_inliers=MIN_INLIERS, min_hull=MIN_HULL_RATIO):
    """loop_closer.cpp:463-479: enough inliers and the inlier pixels' hull covers min_hull of the image in both keyframes.
    kq, kc: KP_DTYPE records of the two keyframes; matches: MATCH_DTYPE records; mask: 1 per inlier.  -> (ok, inliers, hull_q, hull_c)"""
    sel = matches[np.asarray(mask[:len(matches)], bool)]
    hq = hull_area(zip(kq["x"][sel["query"]], kq["y"][sel["query"]])) / float(rows * cols)
    hc = hull_area(zip(kc["x"][sel["train"]], kc["y"][sel["train"]])) / float(rows * cols)
    ok = len(sel) >= min_inliers and hq >= min_hull and hc >= min_hull
    return bool(ok), int(len(sel)), hq, hc


def compact_features(feats, bits, level):
    """the records whose bit `level` is set, in order, at the front of every keyframe's row (the others zeroed): on the device"""
    n, cap = bits.shape
    slot = torch.arange(cap, device=bits.device)[None, :]
    keep = (((bits >> level) & 1) != 0) & (slot < feats.counts[:, None])
    order = torch.argsort((~keep).to(torch.uint8), dim=1, stable=True)
    counts = keep.sum(1).to(torch.int32)
    kps = torch.gather(feats.kps, 1, order[:, :, None].expand(-1, -1, feats.kps.shape[2]))
    kps = torch.where((slot < counts[:, None])[:, :, None], kps, torch.zeros_like(kps)).contiguous()
    return Features(kps, counts)


def masked_features(ctx, feats, blocks, K, rows, cols, mask_level, batch=64, segment_k=None, segment_min=None, mask_out=None, max_segments=None):
    """segment the keyframes (rgbid.segment), mark every keypoint with its mask bits and keep those of mask `mask_level`"""
    from . import segment as SG
    if not 0 < int(mask_level) < SG.DEFAULT_LEVELS:
        raise ValueError(f"mask_level must lie in [0, {SG.DEFAULT_LEVELS}), got {mask_level!r}")
    if blocks is None or len(blocks) != len(feats):
        raise ValueError("mask_level > 0 needs the packed export block of every keyframe (blocks, or overlap_mask and normals in the keyframes)")

    def bits_of(sg, s, res):
        return sg.mask_keypoints(res[4], res[5], feats.kps[s:s + batch].contiguous(), feats.counts[s:s + batch].contiguous())
    bits = torch.cat(SG.segment_batches(ctx, blocks, K, rows, cols, batch, max_segments, bits_of, k=segment_k, min_size=segment_min))
    out = compact_features(feats, bits, int(mask_level))
    if mask_out is not None:
        kps, counts = out.numpy()
        mask_out.update(bits=bits.cpu().numpy(), kps=kps, counts=counts)
    return out


def appearance_loops(ctx, keyframes, K, grey=None, max_keypoints=1000, min_separation=3, score_threshold=SCORE_THRESHOLD, per_query=(2, 2),
                     batch=64, levels=1, scale=SCALE, proposal="match", vocabulary=None, shortlist_size=8, mask_level=0, blocks=None,
                     segment_k=None, segment_min=None, mask_out=None, max_segments=None):
    """features of all exported keyframes, `propose`, RANSAC and its gates.  keyframes: [dict(frame, depthinv, colors)] in export order.
    -> (pairs [(q, c)] that passed, guesses [(R, t)] = qTc_ini of each, report [dict(query, candidate, score, matches, inliers, hull_query,
    hull_candidate, ransac_ok)] over every proposed pair).  levels, scale: the feature pyramid (LoopFeat); the reference runs 8 levels at 1.2.
    proposal: "match" matches every pair; "bow" matches the shortlist_size candidates per keyframe that `vocabulary` ranks best, and the
    report gains bow_score and bow_rank.  vocabulary: a rgbid.bow.Vocabulary; None: one of the default size trained on these keyframes'
    features; a path: the .npz of rgbid.bow.load when the file exists, otherwise one trained on these features and saved there.
    mask_level m > 0: matching and the shortlist see only the keypoints that negentropy mask m of the keyframe keeps (rgbid.segment;
    the reference's masked descriptors); it needs blocks, the packed export block of every keyframe (CUDA uint8 tensors or
    rgbid.cloud Source records); segment_k, segment_min, max_segments: the segmenter's k, smallest segment and the segments per
    keyframe its tables start with (rgbid.segment.segment_batches).  The records are compacted on the
    device, keypoint indices in the results count the kept records.  mask_out (a dict) receives bits [n, max_keypoints] uint8 and the
    compacted kps / counts as numpy.  mask_level 0 changes nothing."""
    import os
    from .posegraph import grey_from_colors
    if proposal not in ("match", "bow"):
        raise ValueError(f'proposal must be "match" or "bow", got {proposal!r}')
    if proposal == "match" and vocabulary is not None:
        raise ValueError('a vocabulary needs proposal="bow"')
    if len(keyframes) < 2:
        return [], [], []
    rows, cols = keyframes[0]["depthinv"].shape
    if grey is None:
        grey = [grey_from_colors(k["colors"]) for k in keyframes]
    lf = LoopFeat(ctx, rows, cols, max_keypoints, levels, scale)
    try:
        parts = [lf.extract(np.stack(grey[s:s + batch]), np.stack([k["depthinv"] for k in keyframes[s:s + batch]]), K)
                 for s in range(0, len(keyframes), batch)]   # records do not depend on the batch
        feats = Features(torch.cat([p.kps for p in parts]), torch.cat([p.counts for p in parts]))
        if mask_level:
            if blocks is None and all("normals" in k and "overlap_mask" in k for k in keyframes):
                blocks = [torch.from_numpy(np.concatenate([np.ascontiguousarray(k[f]).reshape(-1).view(np.uint8) for f in
                                                           ("overlap_mask", "colors", "depthinv", "normals")])).to(f"cuda:{ctx.device}")
                          for k in keyframes]
            feats = masked_features(ctx, feats, blocks, K, rows, cols, mask_level, batch, segment_k, segment_min, mask_out, max_segments)
        voc, own, details = vocabulary, False, {}
        if proposal == "bow" and (voc is None or isinstance(voc, (str, os.PathLike))):
            from . import bow as BW
            own = True
            if voc is not None and os.path.exists(voc):
                voc = BW.load(ctx, voc)
            else:
                path, voc = voc, BW.Vocabulary(ctx)
                try:
                    voc.train(feats)
                    if path is not None:
                        voc.save(path)
                except Exception:
                    voc.close()
                    raise
        try:
            pairs, scores = propose(lf, feats, min_separation, score_threshold, per_query, shortlist=voc, shortlist_size=shortlist_size,
                                    details=details)
        finally:
            if own:
                voc.close()
        if not pairs:
            return [], [], []
        m, mc = lf.match(feats, pairs)
        res = lf.ransac(feats, pairs, m, mc)
        kps, _ = feats.numpy()
        mh, mch = m.cpu().numpy().view(MATCH_DTYPE).reshape(len(pairs), -1), mc.cpu().numpy()
    finally:
        lf.close()
    good, guess, report = [], [], []
    for k, (q, c) in enumerate(pairs):
        mm = mh[k, :mch[k]]
        ok, inl, hq, hc = gate(kps[q], kps[c], mm, res["mask"][k], rows, cols) if res["best"][k] >= 0 else (False, 0, 0.0, 0.0)
        report.append(dict(query=q, candidate=c, score=scores[(q, c)], matches=int(mch[k]), inliers=inl, hull_query=hq, hull_candidate=hc,
                           ransac_ok=ok))
        if details:
            rank = [int(v) for v in details["candidates"][q]].index(c)
            report[-1].update(bow_score=int(details["bow_scores"][q][rank]) / float(1 << 30), bow_rank=rank)
        if ok:
            good.append((q, c))
            guess.append((res["R"][k].copy(), res["t"][k].copy()))
    return good, guess, report
