"""GPU tests of the appearance loop stage end to end: sequence.track_chunked(loops="appearance") on the bounded synthetic path with the
gathered trajectory displaced (a drift that grows along the run, and a jump after the first chunk), where the distance-based proposal
(loops="auto") finds nothing; and
tools/track_dataset.py --loops appearance."""
import os
import subprocess
import sys

import numpy as np
import pytest

from rgbid import posegraph as PG
from rgbid import sequence, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_SMALL = (synth.TUM_K[0] / 4, synth.TUM_K[1] / 4, (synth.TUM_K[2] + 0.5) / 4 - 0.5, (synth.TUM_K[3] + 0.5) / 4 - 0.5)
SHIFT, TURN = np.array([1.0, 0.0, 0.0]), 0.3      # metres, radians after the first chunk: beyond the distance proposal's 0.5 m radius
DRIFT = np.array([0.01, 0.0, 0.0])                # metres per frame over the whole run: keyframes 3 apart (>= 60 frames) end up > 0.5 m apart


def _ate(t, seq):
    gt = seq["t_wc"].cpu().numpy()
    return float(np.sqrt(np.mean(np.sum((np.asarray(t) - gt) ** 2, 1))))


def _displaced(monkeypatch, seam_holder):
    """wrap posegraph.optimise_run: pose k gets k * DRIFT added, and every pose after the first chunk's last frame also SHIFT and a turn by
    TURN about the world z axis, before the graph is built (the measurements stay as tracked: this is a trajectory that has drifted).
    The jump alone leaves the loops inside a chunk within the distance proposal's reach (measured: 3 accepted, none across the seam); the
    drift removes those too, so that what loops="auto" accepts is exactly nothing."""
    orig = PG.optimise_run
    c, s = np.cos(TURN), np.sin(TURN)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])

    def wrapped(ctx, R, t, chunk_records, first_frames, headers, keyframes, K, optimise="auto", loops=None, **kw):
        seam = sorted(first_frames)[1]
        R, t = np.array(R, np.float64), np.array(t, np.float64)
        R[seam + 1:] = Rz @ R[seam + 1:]
        t[seam + 1:] = t[seam + 1:] + SHIFT
        t += np.arange(len(t))[:, None] * DRIFT
        seam_holder["t"], seam_holder["seam"] = t.copy(), seam
        return orig(ctx, R, t, chunk_records, first_frames, headers, keyframes, K, optimise, loops, **kw)
    monkeypatch.setattr(PG, "optimise_run", wrapped)


def test_appearance_closes_loops_under_drift(ctx, monkeypatch):
    """600 frames of the bounded path at 160 x 120 in 2 chunks, the poses drifting by 1 cm per frame and the second chunk's displaced by 1 m and
    0.3 rad.  loops="auto" accepts no loop (every candidate is farther than its radius); loops="appearance" accepts loops, its RANSAC poses
    agree with the ground truth to the dense gate, and the trajectory error falls below the displaced run's."""
    rows, cols, n = 120, 160, 600
    seq = synth.make_long_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda")
    depth, rgb = seq["depth"].contiguous(), seq["rgb"].contiguous()
    hold = {}
    _displaced(monkeypatch, hold)
    R1, t1, _ = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, optimise="auto", loops="auto")
    auto = sequence.track_chunked.last_optimise
    seam = hold["seam"]
    a_disp = _ate(hold["t"], seq)
    a_auto = _ate(t1, seq)
    R2, t2, _ = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, optimise="auto", loops="appearance")
    app = sequence.track_chunked.last_optimise
    a_app = _ate(t2, seq)
    print(f"seam frame {seam}; displaced ATE {a_disp * 1e3:.1f} mm; auto: proposed {len(auto['loops'])}, accepted {auto['accepted']}, ATE {a_auto * 1e3:.1f} mm; "
          f"appearance: proposed {len(app['appearance'])}, RANSAC ok {len(app['loops'])}, accepted {app['accepted']}, ATE {a_app * 1e3:.1f} mm")
    for a in app["appearance"]:
        print("  ", {k: (round(v, 3) if isinstance(v, float) else v) for k, v in a.items()})
    lc = [e for e in auto["edges"] if e["type"] == PG.LC_KF]
    cross_auto = [e for e in lc if (int(e["from"]) > seam) != (int(e["to"]) > seam)]
    print(f"auto: {len(lc)} loop edges, {len(cross_auto)} across the seam")
    assert auto["accepted"] == 0
    assert app["status"] == PG.OK and app["accepted"] >= 1
    # the accepted RANSAC poses against the ground truth's relative poses, to the dense gate
    Rg, tg = seq["R_wc"].cpu().numpy(), seq["t_wc"].cpu().numpy()
    lc_app = [e for e in app["edges"] if e["type"] == PG.LC_KF]
    rows_ok = [r for r in app["loops"] if r["accepted"]]
    assert len(lc_app) == len(rows_ok)
    for e, r in zip(lc_app, rows_ok):
        a, b = int(e["from"]), int(e["to"])
        Rrel, trel = Rg[a].T @ Rg[b], Rg[a].T @ (tg[b] - tg[a])
        R0, t0 = r["guess"]
        dt, dr = float(np.linalg.norm(t0 - trel)), PG._rot_angle(R0.T @ Rrel)
        print(f"   loop {a} <- {b}: RANSAC vs truth {dt * 1e3:.1f} mm, {dr * 1e3:.1f} mrad; inliers {r['inliers']}, score {r['score']:.2f}")
        assert dt <= 0.1 and dr <= 0.1, (a, b, dt, dr)
        assert set(("score", "matches", "inliers", "hull_query", "hull_candidate")) <= set(r)
    assert a_app < a_disp


def test_track_dataset_appearance_option(ctx, tmp_path):
    """--loops appearance runs and reports; without the flag the tool writes the bytes it wrote before"""
    from tests.test_gpu_cloud import write_tum_folder
    rows, cols, n = 120, 160, 40
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    outs = []
    for name, extra in (("plain", []), ("opt", ["--optimise"]), ("app", ["--optimise", "--loops", "appearance"]), ("plain2", [])):
        out = tmp_path / f"{name}.txt"
        r = subprocess.run(base + ["--out", str(out)] + extra, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append((out.read_bytes(), r.stdout))
    assert outs[0][0] == outs[3][0]
    assert "pose graph:" in outs[2][1] and "pose graph:" not in outs[0][1]
    assert len([l for l in outs[2][0].decode().split("\n") if l and not l.startswith("#")]) == n
    print(outs[2][1].strip().split("\n")[-3:])
