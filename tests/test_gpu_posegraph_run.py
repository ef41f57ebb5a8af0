"""GPU tests of the pose-graph back-end's user-facing layers: the C++ drop-in against the C-ABI, sequence.track_chunked(optimise=, loops=)
end to end on a synthetic sequence that revisits its start, and tools/track_dataset.py --optimise --loops auto."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import posegraph as PG
from rgbid import sequence, synth
from tests import pg_mirror as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_SMALL = (synth.TUM_K[0] / 4, synth.TUM_K[1] / 4, (synth.TUM_K[2] + 0.5) / 4 - 0.5, (synth.TUM_K[3] + 0.5) / 4 - 0.5)


def test_cpp_pose_graph_equals_c_abi(ctx, tmp_path):
    """RGBID_SLAM::PoseGraph (buildGraph / optimiseGraph / updatePosesAndKeyframes) gives the C-ABI's poses bit for bit, and re-anchors a pose
    the graph does not hold on the optimised last pose"""
    lib = os.path.join(ROOT, "rgbid-slam_amd", "lib")
    exe = str(tmp_path / "pose_graph_dropin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pose_graph_dropin.cpp"),
                           "-L" + lib, "-lrgbid_host", "-lrgbid_hip", "-Wl,-rpath," + lib, "-o", exe])
    r = np.random.default_rng(4)
    P, E, _ = M.make_graph(r, 80, K=8, L=3, lost=(30,), drift=0.01, noise=1e-4)
    ids = 100 + 3 * np.arange(len(P))                 # pose ids need not be vertex indices
    pg = PG.PoseGraph(ctx)
    try:
        for ml in (True, False):
            src = tmp_path / "graph.bin"
            with open(src, "wb") as f:
                f.write(np.array([len(P), len(E)], np.int32).tobytes())
                for k in range(len(P)):
                    f.write(np.int32(ids[k]).tobytes() + P[k].tobytes())
                for e in E:
                    f.write(np.array([ids[e["from"]], ids[e["to"]], e["type"]], np.int32).tobytes() + e["R"].tobytes() + e["t"].tobytes() + e["cov"].tobytes())
            dst = tmp_path / "out.bin"
            res = subprocess.run([exe, str(src), str(dst), "1" if ml else "0"], capture_output=True, text=True, timeout=300)
            assert res.returncode == 0, res.stdout + res.stderr
            raw = dst.read_bytes()
            st, ok = np.frombuffer(raw[:8], np.int32)
            chi = np.frombuffer(raw[8:24], np.float64)
            got = np.frombuffer(raw[24:], np.float64).reshape(len(P) + 1, 12)
            out, status, chi2 = pg.optimise([(P, E)], multilevel=ml)
            assert st == PG.OK and ok == 1 and status[0] == PG.OK
            assert np.array_equal(got[:-1], out[0]) and np.array_equal(chi, chi2[0])
            # the extra pose: T_last_before * (0.1 m along its x); after the update T_last_after * the same delta
            Ra, ta = out[0][-1, :9].reshape(3, 3), out[0][-1, 9:]
            assert np.allclose(got[-1, :9].reshape(3, 3), Ra, atol=1e-12) and np.allclose(got[-1, 9:], ta + 0.1 * Ra[:, 0], atol=1e-12)
    finally:
        pg.close()


def _ate(R, t, seq):
    gt = seq["t_wc"].cpu().numpy()
    return float(np.sqrt(np.mean(np.sum((np.asarray(t) - gt) ** 2, 1))))


def test_track_chunked_optimise_with_loops(ctx):
    """600 frames of the bounded path (periods ~280 - 520 frames: the camera comes back near its start) at 160 x 120 in 2 chunks:
    optimise="auto", loops="auto" accepts loops and the trajectory error is no worse than without the back-end.  Measured: multilevel, 21 of 21
    loops accepted, ATE 4.16 mm -> 1.99 mm"""
    rows, cols, n = 120, 160, 600
    seq = synth.make_long_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda")
    depth, rgb = seq["depth"].contiguous(), seq["rgb"].contiguous()
    R0, t0, ranges = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL)
    R1, t1, ranges1 = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, optimise="auto", loops="auto")
    info = sequence.track_chunked.last_optimise
    a0, a1 = _ate(R0, t0, seq), _ate(R1, t1, seq)
    print(f"pose graph: mode {info['mode']}, status {info['status']}, chi2 {info['chi2'][0]:.4g} -> {info['chi2'][1]:.4g}, loops accepted "
          f"{info['accepted']} of {len(info['loops'])}; ATE {a0 * 1e3:.2f} mm -> {a1 * 1e3:.2f} mm")
    assert ranges1 == ranges and R1.shape == R0.shape
    assert info["status"] == PG.OK and info["mode"] in ("multilevel", "single")
    assert info["accepted"] >= 1
    assert a1 <= a0 * 1.0 + 1e-4
    # the defaults are unchanged byte for byte
    R2, t2, _ = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL)
    assert np.array_equal(R2, R0) and np.array_equal(t2, t0)


def test_track_dataset_optimise_option(ctx, tmp_path):
    from tests.test_gpu_cloud import write_tum_folder
    rows, cols, n = 120, 160, 40
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    out = tmp_path / "traj.txt"
    r = subprocess.run(base + ["--out", str(out), "--optimise", "--loops", "auto"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "pose graph:" in r.stdout and len([l for l in out.read_text().split("\n") if l and not l.startswith("#")]) == n
    print(r.stdout.strip().split("\n")[-2])
