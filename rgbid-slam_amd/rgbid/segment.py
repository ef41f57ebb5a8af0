"""Superjut segmentation of keyframes and the negentropy masks of loop features (binding of include/rgbid_segment.h).

The reference cuts every new keyframe's cloud into "superjuts" (a Felzenszwalb-style graph segmentation over pixel-neighbour edges
weighted by normal curvature), gives every segment the entropy of its histogram of normals, and masks the loop-closure keypoints that
lie on low-information surfaces (walls, floors, table tops).  `Segmenter.segment` does that on the device for a batch of keyframes in
the engine's packed export layout and returns labels, segment tables, the negentropy image and the mask levels, bitwise reproducible
(DESIGN.md section 16); `Segmenter.mask_keypoints` turns them into one byte of mask bits per `rgbid.loopfeat` keypoint record.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, ci, f32, vp
from .cloud import Source, source

MAX_BINS, DEFAULT_BINS = 128, 80
MAX_LEVELS, DEFAULT_LEVELS = 8, 4
MAX_WINDOW = 256
DEFAULT_K, DEFAULT_MIN_SIZE = 0.6, 300
THRESHOLDS = np.array([0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9], np.float32)
SIGNATURES = {
    "rgbid_segment_create": (vp, vp, ci, ci, ci, ci),
    "rgbid_segment_destroy": (vp,),
    "rgbid_segment_workspace_bytes": (ci, ci, ci, ci, vp),
    "rgbid_segment_device_bytes": (vp, vp),
    "rgbid_segment_bins": (ci, vp),
    "rgbid_segment_set_window": (vp, ci),
    "rgbid_segment_run": (vp, ci, vp, vp, f32, ci, ci, ci, vp, vp, vp, vp, vp, vp),
    "rgbid_segment_mask_keypoints": (vp, vp, vp, ci, ci, vp, vp, ci, vp),
    "rgbid_segment_last_rounds": (vp, vp),
    "rgbid_segment_timing": (vp, ci, vp),
}
EXPORTS = list(SIGNATURES)
STAGES = ("edges", "sort", "pass1", "pass2", "labels", "histogram")


def bins(nbins=DEFAULT_BINS):
    """the bin centres of the histogram of normals, float32 [nbins, 3] (needs no device)"""
    out = np.zeros((int(nbins), 3), np.float32)
    check(_lib.bind(SIGNATURES).rgbid_segment_bins(int(nbins), out.ctypes.data_as(C.c_void_p)))
    return out


def workspace_bytes(rows, cols, max_keyframes, max_segments):
    """device bytes a Segmenter of these arguments allocates (needs no device)"""
    b = C.c_ulonglong()
    check(_lib.bind(SIGNATURES).rgbid_segment_workspace_bytes(int(rows), int(cols), int(max_keyframes), int(max_segments), C.byref(b)))
    return b.value


class SegmentOverflow(ValueError):
    """a keyframe has more segments (`count`) than the Segmenter's tables hold"""

    def __init__(self, count, max_segments):
        super().__init__(f"a keyframe has {count} segments, the tables hold {max_segments}: create the Segmenter with max_segments >= {count}")
        self.count = int(count)


def blocks_of(blocks):
    """`blocks`: rgbid.cloud Source records, or CUDA uint8 tensors holding one packed export block each -> a list of Source"""
    out = []
    for b in blocks:
        if isinstance(b, Source):
            out.append(b)
        else:
            assert isinstance(b, torch.Tensor) and b.is_cuda and b.dtype == torch.uint8 and b.is_contiguous(), "a block: a contiguous CUDA uint8 tensor"
            out.append(source(b.data_ptr(), np.eye(3), np.zeros(3)))
    return out


class Segmenter(_lib.CtxHandle):
    """Segmenter for keyframes of rows x cols pixels, up to max_keyframes per call, with tables for max_segments segments per keyframe
    (default: min(rows cols, 4096)), on the context's stream."""
    _destroy, _signatures, _timing, _stages = "rgbid_segment_destroy", SIGNATURES, "rgbid_segment_timing", STAGES

    def __init__(self, ctx, rows, cols, max_keyframes, max_segments=None, k=DEFAULT_K, min_size=DEFAULT_MIN_SIZE, nbins=DEFAULT_BINS,
                 levels=DEFAULT_LEVELS):
        super().__init__(ctx)
        self.rows, self.cols, self.max_keyframes = int(rows), int(cols), int(max_keyframes)
        self.max_segments = int(max_segments) if max_segments is not None else min(self.rows * self.cols, 4096)
        self.k, self.min_size, self.nbins, self.levels = float(k), int(min_size), int(nbins), int(levels)
        self._created(self.L.rgbid_segment_create(C.byref(self._h), ctx._h, self.rows, self.cols, self.max_keyframes, self.max_segments))

    def set_window(self, window):
        """test hook: the window of the union-find rounds (1 .. 256); no window changes a result"""
        check(self.L.rgbid_segment_set_window(self._h, int(window)))

    def segment(self, blocks, K, k=None, min_size=None, nbins=None, levels=None):
        """-> labels int32 [n, rows, cols], counts int32 [n], sizes int32 [n, max_segments], hist int32 [n, max_segments, nbins],
        negentropy float32 [n, rows, cols], mask_levels int32 [n, levels]: CUDA tensors.  The blocks must stay valid and unchanged until
        this returns (it synchronises).  SegmentOverflow (a ValueError) when a keyframe has more than max_segments segments."""
        srcs = blocks_of(blocks)
        n = len(srcs)
        k = self.k if k is None else float(k)
        min_size = self.min_size if min_size is None else int(min_size)
        nbins = self.nbins if nbins is None else int(nbins)
        levels = self.levels if levels is None else int(levels)
        dev = self._dev
        i32 = dict(dtype=torch.int32, device=dev)
        labels = torch.empty((n, self.rows, self.cols), **i32)
        counts = torch.empty((n,), **i32)
        sizes = torch.empty((n, self.max_segments), **i32)
        hist = torch.empty((n, self.max_segments, max(nbins, 1)), **i32)
        neg = torch.empty((n, self.rows, self.cols), dtype=torch.float32, device=dev)
        lev = torch.empty((n, max(levels, 1)), **i32)
        arr = (Source * max(n, 1))(*srcs)
        kk = (C.c_float * 4)(*[float(v) for v in K])
        self.ctx.wait_torch_stream()   # the blocks and the outputs are torch's allocations
        check(self.L.rgbid_segment_run(self._h, n, arr, kk, C.c_float(k), min_size, nbins, levels, *[C.c_void_p(t.data_ptr()) for t in
                                                                                                     (labels, counts, sizes, hist, neg, lev)]))
        self.ctx.sync()
        most = int(counts.max())
        if most > self.max_segments:
            raise SegmentOverflow(most, self.max_segments)
        return labels, counts, sizes, hist, neg, lev

    def mask_keypoints(self, negentropy, mask_levels, kps, counts):
        """negentropy [n, rows, cols] and mask_levels [n, M] of a segment() call, kps uint8 [n, max_keypoints, 120] and counts int32 [n] of a
        rgbid.loopfeat extraction -> CUDA uint8 [n, max_keypoints]: bit m is set when mask m keeps the keypoint's pixel.  Synchronises."""
        n, M = mask_levels.shape
        assert negentropy.shape == (n, self.rows, self.cols) and negentropy.dtype == torch.float32 and negentropy.is_contiguous()
        assert mask_levels.dtype == torch.int32 and mask_levels.is_contiguous() and counts.dtype == torch.int32 and counts.shape == (n,)
        assert kps.dtype == torch.uint8 and kps.is_contiguous() and kps.dim() == 3 and kps.shape[0] == n and kps.shape[2] == 120
        bits = torch.empty((n, kps.shape[1]), dtype=torch.uint8, device=kps.device)
        self.ctx.wait_torch_stream()
        check(self.L.rgbid_segment_mask_keypoints(self._h, negentropy.data_ptr(), mask_levels.data_ptr(), n, M, kps.data_ptr(), counts.data_ptr(),
                                                  kps.shape[1], bits.data_ptr()))
        self.ctx.sync()
        return bits

    def device_bytes(self):
        """the device bytes this handle holds: workspace_bytes of its arguments"""
        b = C.c_ulonglong()
        check(self.L.rgbid_segment_device_bytes(self._h, C.byref(b)))
        return b.value

    def last_rounds(self):
        """-> (pass 1, pass 2): the most rounds a keyframe of the last segment() call needed"""
        r = (C.c_ulonglong * 2)()
        check(self.L.rgbid_segment_last_rounds(self._h, r))
        return int(r[0]), int(r[1])

DEFAULT_MAX_SEGMENTS = 4096


def segment_batches(ctx, blocks, K, rows, cols, batch=16, max_segments=None, use=None, **params):
    """segment any number of keyframes `batch` at a time with one Segmenter whose tables start at max_segments (default min(rows cols,
    4096)); a batch with a keyframe of more segments is run again with tables of that count (isolated points have no edge, so no
    min_size bounds the count).  use(segmenter, first, outputs) is called per batch and its results are returned as a list; params: k,
    min_size, nbins, levels (None: the default)."""
    S = min(rows * cols, int(max_segments) if max_segments is not None else DEFAULT_MAX_SEGMENTS)
    params = {k: v for k, v in params.items() if v is not None}
    out, s = [], 0
    sg = Segmenter(ctx, rows, cols, min(batch, len(blocks)), S, **params)
    try:
        while s < len(blocks):
            try:
                res = sg.segment(blocks[s:s + batch], K)
            except SegmentOverflow as e:
                sg.close()
                S = min(rows * cols, e.count)
                sg = Segmenter(ctx, rows, cols, min(batch, len(blocks)), S, **params)
                continue
            out.append(use(sg, s, res) if use else res)
            s += batch
    finally:
        sg.close()
    return out
