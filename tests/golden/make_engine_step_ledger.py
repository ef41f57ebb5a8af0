"""Generates tests/golden/engine_step_ledger.json: the launch count (Engine.launches_per_step) and the four byte buckets (Engine.step_bytes) of the
engine's step for a matrix of geometries and configurations, after step 1 (the first-frame list) and after step 3 (the steady list).  These are the
project's own numbers: they pin what bench.py reports (launches per step, the roofline fraction's byte model) while the code that builds the launch list
is rearranged.  tests/test_gpu_engine.py::test_engine_step_ledger_matches_recorded imports MATRIX and record() from here and compares with the file.

    python tests/golden/make_engine_step_ledger.py [--commit HASH] [--out FILE]      (needs the GPU; run from the repo root at the commit to be recorded)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "rgbid-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

LEDGER = os.path.join(ROOT, "tests", "golden", "engine_step_ledger.json")
LANES = 2
# 120x160 with 3 levels: every vectorised path.  122x166 with 2 levels: cols % 4 != 0 -- the Sobel-and-copy pass, the keyframe-map kernel, the fusion kernel
# and the frame converter take their fallbacks
GEOMETRIES = [(120, 160, 3), (122, 166, 2)]


def configurations(levels):
    """name -> (engine configuration keywords, environment).  Named as in test_engine_configurations where that test has the configuration."""
    from oracle import oracle as O
    zero = dict(iters=[4, 0, 3]) if levels == 3 else dict(iters=[0, 4])
    fin1 = dict(finest_level=1, iters=[0, 6, 4]) if levels == 3 else dict(finest_level=1, iters=[0, 4])
    return [
        ("default", dict(), {}),
        ("fast_numerics=0", dict(fast_numerics=0), {}),
        ("fused_gn=0", dict(fused_gn=0), {}),
        ("warp first", dict(warping=O.WARP_FIRST), {}),
        ("chi-squared termination, pyr first (stale level-0 maps)", dict(termination=O.CHI_SQUARED, warping=O.PYR_FIRST, fast_numerics=0), {}),
        ("chi-squared termination, warp first", dict(termination=O.CHI_SQUARED, warping=O.WARP_FIRST, fast_numerics=0), {}),
        ("Huber + sigma const + min weight", dict(mestimator=O.HUBER, sigma_estimator=O.SIGMA_CONS, weighting=O.MIN_WEIGHT), {}),
        ("Tukey + filtered gradients + no motion model", dict(mestimator=O.TUKEY, image_filtering=O.FILTER_GRADS, motion_model=O.NO_MM), {}),
        ("chi_square_stats=1", dict(chi_square_stats=1), {}),
        ("preview=1", dict(preview=1), {}),
        ("keyframe export", dict(keyframe_capacity=3, defer_keyframe_maps=0), {}),
        ("keyframe export, deferred maps", dict(keyframe_capacity=3, defer_keyframe_maps=1), {}),
        ("custom_registration=1", dict(custom_registration=1), {}),
        ("a level of zero iterations", zero, {}),
        ("finest level 1", fin1, {}),
        ("default, update prologue off", dict(), {"RGBID_ENGINE_UPDATE_PROLOGUE_LANES": "0"}),
    ]


def matrix():
    """[(key, rows, cols, levels, use_graph, cfg_kw, env)]: every configuration eagerly, the default also as a replayed graph"""
    out = []
    for rows, cols, levels in GEOMETRIES:
        for name, kw, env in configurations(levels):
            for use_graph in ((0, 1) if name == "default" else (0,)):
                out.append((f"{rows}x{cols} L{levels} | {name} | use_graph={use_graph}", rows, cols, levels, use_graph, kw, env))
    return out


def _config(rows, cols, levels, use_graph, kw):
    from rgbid import _lib, engine as E
    from rgbid.device import IntrK, depth_dist
    s = cols / 640.0
    K = (525.0 * s, 525.0 * s, (319.5 + 0.5) * s - 0.5, (239.5 + 0.5) * rows / 480.0 - 0.5)
    kw = dict(kw)
    if "iters" not in kw:
        kw["iters"] = [10, 5, 3][:levels]
    cfg = E.default_config(rows=rows, cols=cols, levels=levels, lanes=LANES, K=K, use_graph=use_graph, record_capacity=3, **kw)
    if kw.get("custom_registration"):   # the calibration of test_engine_custom_calibration, scaled to the image
        for i, v in enumerate((0.02, -0.04, 0.0005, -0.0004, 0.01)):
            cfg.rgb_dist[i] = v
        cfg.depth_intr = IntrK(571.0 * s, 572.5 * s, 316.0 * s, 241.5 * s, -0.015, 0.03, 0.0003, 0.0002, -0.008)
        cfg.depth_dist = depth_dist(c1=1.01, c0=-0.002, q0=(0.001, -0.002, 0.001, 0.0, 0.0005, -0.0004, 0.0, 0.0, 0.0), q1=(0.005, 0.01, 0.0, 0.0, -0.002, 0.001, 0.0, 0.0, 0.0))
        dRc = [0.99995, -0.008, 0.006, 0.00803, 0.99995, -0.005, -0.00596, 0.00505, 0.99997]
        _lib.check(_lib.lib().rgbid_engine_config_set_stereo(C.byref(cfg), (C.c_float * 9)(*dRc), (C.c_float * 3)(0.0251, -0.0012, 0.0031)))
    return cfg, K


def record(ctx):
    """key -> {"first": {"launches", "bytes"}, "steady": {...}}: the ledger of every entry of the matrix, three steps per engine"""
    import torch
    from rgbid import engine as E, synth
    frames = {}
    out = {}
    for key, rows, cols, levels, use_graph, kw, env in matrix():
        cfg, K = _config(rows, cols, levels, use_graph, kw)
        if (rows, cols) not in frames:
            seqs = [synth.make_sequence(3, seed=synth.SEED + 17 * l, K=K, rows=rows, cols=cols, device="cuda") for l in range(LANES)]
            frames[(rows, cols)] = (torch.stack([s["depth"] for s in seqs], 1).to(torch.int16).contiguous(), torch.stack([s["rgb"] for s in seqs], 1).contiguous())
        depth, rgb = frames[(rows, cols)]
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            eng = E.Engine(ctx, cfg)
            entry = {}
            for k in range(3):
                eng.step(depth[k], rgb[k])
                if k in (0, 2):
                    b = eng.step_bytes()
                    assert all(float(v).is_integer() for v in b), (key, b)     # integer coefficients times pixel / sample counts
                    entry["first" if k == 0 else "steady"] = {"launches": int(eng.launches_per_step()), "bytes": [int(v) for v in b]}
            eng.records()
            eng.close()
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        out[key] = entry
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the numbers are recorded at (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=LEDGER)
    a = ap.parse_args()
    commit = a.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    from rgbid import device
    ctx = device.Context(0)
    entries = record(ctx)
    ctx.close()
    with open(a.out, "w") as f:
        json.dump({"recorded_at_commit": commit, "lanes": LANES, "bytes": "[every tracked frame, + per odometry-keyframe switch, + per integration-keyframe switch, + per fused frame], per lane",
                   "entries": entries}, f, indent=1)
        f.write("\n")
    print(f"{len(entries)} entries -> {a.out}")


if __name__ == "__main__":
    main()
