"""CPU tests of the segmentation options of tools/track_dataset.py: whatever other loop options are given, the mask and segmenter
options reach the keywords of sequence.track_chunked, and rgbid.posegraph.optimise_run hands them on to appearance_loops."""
import argparse
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("track_dataset_tool", os.path.join(ROOT, "tools", "track_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(**kw):
    base = dict(optimise="auto", loops="appearance", loop_levels=1, loop_scale=1.2, loop_proposal=None, loop_vocabulary=None, loop_shortlist=None,
                loop_mask_level=0, segment_k=None, segment_min=None, segment_max=None, labels_out="")
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.mark.parametrize("extra", [dict(), dict(loop_levels=8), dict(loop_scale=1.5), dict(loop_proposal="bow", loop_shortlist=4),
                                   dict(loop_levels=8, loop_proposal="bow", loop_vocabulary="v.npz")])
def test_mask_options_survive_the_other_loop_options(extra):
    T = _tool()
    opt = T.run_options(_args(loop_mask_level=2, segment_k=0.4, segment_min=200, segment_max=9000, **extra))
    lo = opt["loop_options"]
    assert (lo["mask_level"], lo["segment_k"], lo["segment_min"], lo["max_segments"]) == (2, 0.4, 200, 9000)
    if "loop_levels" in extra or "loop_scale" in extra:
        assert (lo["levels"], lo["scale"]) == (extra.get("loop_levels", 1), extra.get("loop_scale", 1.2))
    if extra.get("loop_proposal") == "bow":
        assert lo["proposal"] == "bow" and lo["vocabulary"] == extra.get("loop_vocabulary")
        assert lo.get("shortlist_size") == extra.get("loop_shortlist")
    without = T.run_options(_args(**extra))
    assert "mask_level" not in without.get("loop_options", {}) and "segment" not in without


def test_labels_option_alone_asks_for_the_segmentation():
    T = _tool()
    opt = T.run_options(_args(optimise=None, loops=None, labels_out="dir", segment_min=100))
    assert opt == dict(segment=dict(k=None, min_size=100, max_segments=None))
    assert T.run_options(_args(optimise=None, loops=None)) == {}


def test_optimise_run_hands_the_mask_options_to_appearance_loops(monkeypatch):
    import numpy as np
    from rgbid import loopfeat, posegraph as PG
    seen = {}

    class Stop(Exception):
        pass

    def capture(ctx, keyframes, K, **kw):
        seen.update(kw)
        raise Stop
    monkeypatch.setattr(loopfeat, "appearance_loops", capture)
    monkeypatch.setattr(PG, "graph_from_run", lambda *a: (np.zeros((0, 7)), np.zeros((0, 30))))
    with pytest.raises(Stop):
        PG.optimise_run(None, None, None, [], [], [], [], (1, 1, 0, 0), "auto", "appearance", mask_level=2, segment_k=0.5, segment_min=7,
                        max_segments=99, blocks=["b"], levels=8)
    assert (seen["mask_level"], seen["segment_k"], seen["segment_min"], seen["max_segments"], seen["blocks"], seen["levels"]) == (2, 0.5, 7, 99, ["b"], 8)
