"""GPU tests of the segmenter inside a tracked run and of its bench tool: sequence.track_chunked(segment=...) alone exports keyframes
and labels each as rgbid.segment.Segmenter labels the same ring block; with loops = "appearance" and mask_level the masks read the ring's
blocks; a keyframe with more segments than the tables start with is segmented again; the device bytes of a handle are what
rgbid_segment_workspace_bytes says; tools/segment_bench.py runs at a tiny size."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import cloud as CL
from rgbid import loopfeat as LF
from rgbid import segment as SG
from rgbid import sequence, synth
from tests.test_cpu_segment import K_OF, SIZES, mirror, scenes
from tests.test_gpu_cloud import K_SMALL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tracked_run_labels_and_ring_blocks(ctx, monkeypatch):
    rows, cols, n = 120, 160, 25                                       # 2 chunks of 13 frames each: no lane is padded
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", noise=False, dropout=0.0, trans_step=(0.01, 0.02),
                              rot_step_deg=(0.5, 1.0))
    depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
    kw = dict(visratio_odo=0.985, visratio_integr=0.97)
    sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, segment=dict(min_size=50), **kw)      # nothing else asks for the export ring
    alone = sorted(sequence.track_chunked.last_labels, key=lambda r: (r[0], r[1]))
    assert len(alone) >= 2 and all(l.shape == (rows, cols) and l.dtype == np.int32 and l.max() >= 0 for _, _, l in alone)
    seen = {}
    orig = LF.appearance_loops

    def capture(ctx_, keyframes, K, **akw):
        sg = SG.Segmenter(ctx_, rows, cols, len(akw["blocks"]), rows * cols, min_size=50)     # the engine and its ring are alive here
        try:
            seen.update(akw, labels=sg.segment(akw["blocks"], K)[0].cpu().numpy(), keys=[sorted(k) for k in keyframes])
        finally:
            sg.close()
        info = {}
        out = orig(ctx_, keyframes, K, **dict(akw, mask_out=info))                           # the masks read the ring's blocks
        seen["info"] = info
        return out
    monkeypatch.setattr(LF, "appearance_loops", capture)
    R, t, _ = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, optimise="auto", loops="appearance", segment=dict(min_size=50),
                                     loop_options=dict(mask_level=1, segment_min=50, max_keypoints=300), **kw)
    assert R.shape == (n, 3, 3) and np.isfinite(R).all() and np.isfinite(t).all()             # the run went through the pose graph
    assert sequence.track_chunked.last_optimise["status"] is not None
    assert seen["mask_level"] == 1 and seen["segment_min"] == 50
    assert len(seen["blocks"]) == len(alone) and all(isinstance(b, CL.Source) for b in seen["blocks"])
    assert all(k == ["colors", "depthinv", "frame"] for k in seen["keys"])                    # the keyframes are what they were without masks
    assert seen["info"]["bits"].shape == (len(alone), 300) and (seen["info"]["bits"] & 1).any()
    both = sorted(sequence.track_chunked.last_labels, key=lambda r: (r[0], r[1]))
    assert [r[:2] for r in both] == [r[:2] for r in alone]
    for (_, _, l), (_, _, a), direct in zip(both, alone, seen["labels"]):
        assert np.array_equal(l, a) and np.array_equal(a, direct)      # keyframes in frame order are in (chunk, export) order


def test_tables_grow_to_the_reported_count(ctx):
    s = scenes()["k_zero"]
    rows, cols = SIZES["a"]
    blk = torch.from_numpy(np.ascontiguousarray(s["block"])).cuda()
    m = mirror("k_zero")
    assert m["count"] > 4
    made = []
    res = SG.segment_batches(ctx, [blk, blk, blk], K_OF["a"], rows, cols, batch=2, max_segments=4, k=s["kth"], min_size=s["min_size"],
                             use=lambda sg, first, out: made.append(sg.max_segments) or [t.cpu().numpy() for t in out])
    assert made == [m["count"], m["count"]] and [len(r[0]) for r in res] == [2, 1]
    for r in res:
        for k in range(len(r[0])):
            assert np.array_equal(r[0][k], m["labels"]) and r[1][k] == m["count"] and np.array_equal(r[2][k], m["sizes"])


@pytest.mark.parametrize("args", [(37, 53, 1, 7), (48, 64, 5, 48 * 64), (120, 160, 3, 4096), (120, 160, 14, 4096)])
def test_device_bytes_are_the_sizing(ctx, args):
    sg = SG.Segmenter(ctx, *args)
    try:
        assert sg.device_bytes() == SG.workspace_bytes(*args)
    finally:
        sg.close()


def test_bench_tool_runs_small(tmp_path):
    out = tmp_path / "bench.jsonl"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "segment_bench.py"), "--sizes", "1", "2", "--rows", "48", "--cols", "64",
                           "--reps", "1", "--out", str(out)], timeout=120)
    lines = [json.loads(l) for l in open(out)]
    assert [l["keyframes"] for l in lines] == [1, 2]
    for l in lines:
        assert l["points"] > 0 and l["rounds_pass1"] > 0 and set(l["stage_ms"]) == set(SG.STAGES) and all(v > 0 for v in l["stage_ms"].values())
