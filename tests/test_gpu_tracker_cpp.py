"""GPU parity of the C++ VisodoTracker mirror (librgbid_host.so, host-driven through the bridge API of
include/rgbid/internal.h) against the CPU oracle tracker: pose < 1e-4 rad / 1e-4 m per frame (north star),
identical keyframe decisions, for the shipped configuration and for the non-default modes the engine does not run."""
import numpy as np
import pytest

from oracle import oracle as O
from rgbid import host, synth

pytestmark = pytest.mark.gpu


def rot_angle(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


# the compat tracker in its two modes: host-driven through the bridge (the reference's call sequence), and backed by the one-lane engine
# (VisodoTracker::setEngineBacked: the class default since round 5)
both_modes = pytest.mark.parametrize("engine_backed", [False, True], ids=["host", "engine"])


def run(rows, cols, K, n_frames, cfg_kw, seq_kw, pose_tol=1e-4, map_outliers=5e-3, engine_backed=False):
    seq = synth.make_sequence(n_frames, K=K, rows=rows, cols=cols, device="cuda", **seq_kw)
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    kw = dict(rows=rows, cols=cols, fx=K[0], fy=K[1], cx=K[2], cy=K[3], **cfg_kw)
    trk = host.Tracker(host.default_config(**kw), engine_backed=engine_backed)
    orc = O.Tracker(O.default_config(**kw))
    th_odo, th_int = cfg_kw.get("visratio_odo", 0.9), cfg_kw.get("visratio_integr", 0.7)
    imposed = 0
    for k in range(n_frames):
        a = trk.track(d[k], c[k])
        ia = trk.last_info()
        if k:
            # every frame is compared: where a covisibility ratio lands on its threshold the oracle continues with the product tracker's
            # decision imposed (test hook of the oracle) -- the natural decision may only have differed because the ratio sat on the threshold
            orc.force_kf_decisions(bool(ia.odo_kf_switched), bool(ia.integr_kf_switched))
        b = orc.track(d[k], c[k])
        assert a == b, k
        if k and a:
            ib = orc.last_info()
            assert abs(ia.visratio_odo - ib.visratio_odo) < 5e-4 and ia.nu_depthinv == ib.nu_depthinv   # a handful of pixels at the 0.020 gate may flip
            if bool(ia.odo_kf_switched) != bool(ib.odo_kf_natural):
                assert abs(ib.visratio_odo - th_odo) < 5e-4 and abs(ia.visratio_odo - th_odo) < 5e-4, (k, ia.visratio_odo, ib.visratio_odo)
                imposed += 1
            if bool(ia.integr_kf_switched) != bool(ib.integr_kf_natural):
                assert abs(ib.visratio_integr - th_int) < 5e-4 and abs(ia.visratio_integr - th_int) < 5e-4, (k, ia.visratio_integr, ib.visratio_integr)
                imposed += 1
    if imposed:
        print(f"keyframe decisions on the threshold, imposed on the oracle: {imposed}")
    Ra, ta = trk.poses(); Rb, tb = orc.poses()
    assert len(Ra) == len(Rb)
    for k in range(n_frames):
        assert rot_angle(Ra[k], Rb[k]) < pose_tol and np.linalg.norm(ta[k] - tb[k]) < pose_tol, (k, rot_angle(Ra[k], Rb[k]), np.linalg.norm(ta[k] - tb[k]))
    oa, ota, ca = trk.odometry(); ob, otb, cb = orc.odometry()
    for k in range(1, n_frames):
        sc = np.sqrt(np.outer(np.diag(cb[k]), np.diag(cb[k]))) + 1e-30
        assert (np.abs(ca[k] - cb[k]) / sc).max() < 1e-2
    kd, kw_ = trk.keyframe_maps()
    od = orc.kf_depthinv()
    assert np.count_nonzero(np.isnan(kd) != np.isnan(od)) <= 2e-3 * od.size
    m = ~np.isnan(kd) & ~np.isnan(od)
    rel = np.abs(kd[m] - od[m]) / od[m]          # a few pixels flip the fusion gate / the point-sampled source pixel (cf. test_gpu_engine)
    assert np.count_nonzero(rel > 1e-4) <= max(16, map_outliers * rel.size) and (map_outliers >= 1.0 or np.median(rel) < 1e-5)
    trk.close(); orc.close()


SMALL_K = (131.25, 131.25, 79.5, 59.5)
SLOW = dict(trans_step=(0.003, 0.012), rot_step_deg=(0.1, 0.8))


@both_modes
def test_cpp_tracker_shipped_config(engine_backed):
    run(120, 160, SMALL_K, 6, dict(), SLOW, engine_backed=engine_backed)


@both_modes
def test_cpp_tracker_warp_first(engine_backed):
    run(120, 160, SMALL_K, 4, dict(warping=O.WARP_FIRST), SLOW, engine_backed=engine_backed)


@both_modes
def test_cpp_tracker_filter_grads_and_min_weight(engine_backed):
    run(120, 160, SMALL_K, 4, dict(image_filtering=O.FILTER_GRADS, weighting=O.MIN_WEIGHT), SLOW, engine_backed=engine_backed)


@both_modes
def test_cpp_tracker_sigma_const_no_motion_model(engine_backed):
    run(120, 160, SMALL_K, 4, dict(sigma_estimator=O.SIGMA_CONS, motion_model=O.NO_MM), SLOW, engine_backed=engine_backed)


@both_modes
@pytest.mark.parametrize("warping", [O.WARP_FIRST, O.PYR_FIRST])
def test_cpp_tracker_chi_squared_termination(engine_backed, warping):
    """termination = CHI_SQUARED (visodo.cpp:1134-1164): a level ends, and the last increment is undone, as soon as the full-lattice
    RMSE grows.  With WARP_FIRST the level-0 warped maps the test reads are fresh at every level; with PYR_FIRST (round 6) they are what the last
    level-0 warp left (zero-filled before the first one, in the tracker and in the oracle alike).  Engine-backed (round 5): the stop is a
    per-lane flag written by a decision kernel that masks the rest of the level."""
    kw = dict(warping=warping, termination=O.CHI_SQUARED)
    run(120, 160, SMALL_K, 5, kw, SLOW, engine_backed=engine_backed)
    # the early exit really fires on this sequence: the oracle's trajectory differs from the all-iterations one
    seq = synth.make_sequence(5, K=SMALL_K, rows=120, cols=160, device="cuda", **SLOW)
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    out = []
    for term in (O.CHI_SQUARED, O.ALL_ITERS):
        t = O.Tracker(O.default_config(rows=120, cols=160, fx=SMALL_K[0], fy=SMALL_K[1], cx=SMALL_K[2], cy=SMALL_K[3], warping=warping, termination=term))
        for k in range(5):
            t.track(d[k], c[k])
        out.append(t.poses()[1])
    assert np.abs(out[0] - out[1]).max() > 1e-7


@both_modes
def test_cpp_tracker_keyframe_switches(engine_backed):
    run(120, 160, SMALL_K, 8, dict(visratio_odo=0.985, visratio_integr=0.97), dict(trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0)), engine_backed=engine_backed)


@both_modes
def test_cpp_tracker_full_res(engine_backed):
    run(480, 640, synth.TUM_K, 4, dict(), dict(), engine_backed=engine_backed)


@both_modes
def test_cpp_tracker_four_levels_1280x960(engine_backed):
    """BASELINE config 5: 1280x960 upsampled synthetic stream, 4-level pyramid."""
    K = (1050.0, 1050.0, 639.5, 479.5)
    run(960, 1280, K, 3, dict(levels=4, iters=[10, 5, 3, 3]), dict(), engine_backed=engine_backed)


def _kf_pair(seq, d, c, a, b):
    iD = [O.depth2invdepth(d[k]) for k in (a, b)]
    grey = [np.clip(np.rint(O.intensity(c[k])), 0, 255).astype(np.uint8) for k in (a, b)]
    Rg, tg = [x.numpy() for x in synth.relative_pose(seq["R_wc"][a], seq["t_wc"][a], seq["R_wc"][b], seq["t_wc"][b])]
    return iD, grey, Rg, tg


@pytest.mark.parametrize("host_driven", [True, False], ids=["host", "device-resident"])
def test_keyframe_align_vs_oracle(host_driven):
    """KeyframeAlign (second consumer of the kernels: 4 levels, computeNuStudent, KF-iD sampling grid), in both of its loops: the reference's
    call sequence through the bridge, and (the class default since round 5) the 1-pair case of the device-resident batched aligner."""
    seq = synth.make_sequence(4, device="cuda", trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    iD, grey, Rg, tg = _kf_pair(seq, d, c, 0, 3)
    R, t, cov = host.keyframe_align(iD[0], grey[0], iD[1], grey[1], synth.TUM_K, host_driven=host_driven)
    Ro, to, covo = O.keyframe_align(iD[0], grey[0], iD[1], grey[1], synth.TUM_K)
    assert rot_angle(R, Ro) < 1e-4 and np.linalg.norm(t - to) < 1e-4, (rot_angle(R, Ro), np.linalg.norm(t - to))
    sc = np.sqrt(np.outer(np.diag(covo), np.diag(covo)))
    assert (np.abs(cov - covo) / sc).max() < 1e-2
    assert rot_angle(R, Rg) < 3e-3 and np.linalg.norm(t - tg) < 1e-2     # and it finds the true relative pose


def test_keyframe_align_device_resident_equals_host_driven():
    """the 1-pair case of rgbid_kfalign_batched runs the same kernels in the same order as the host-driven KeyframeAlign: pose and covariance IDENTICAL"""
    seq = synth.make_sequence(4, device="cuda", trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    iD, grey, _, _ = _kf_pair(seq, d, c, 0, 3)
    a = host.keyframe_align(iD[0], grey[0], iD[1], grey[1], synth.TUM_K, host_driven=True)
    b = host.keyframe_align(iD[0], grey[0], iD[1], grey[1], synth.TUM_K, host_driven=False)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_keyframe_align_follows_the_interpolation_mode_in_both_loops():
    """the device-resident aligner runs on a context of its own; it must sample like the thread's default context (VisodoTracker::setInterpMode),
    which the host-driven loop uses -- with the exact bilinear mode selected both loops still agree bit for bit, and differ from the TEX8 result"""
    seq = synth.make_sequence(4, device="cuda", trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    iD, grey, _, _ = _kf_pair(seq, d, c, 0, 3)
    L = host.lib()
    tex8 = host.keyframe_align(iD[0], grey[0], iD[1], grey[1], synth.TUM_K, host_driven=False)
    host.check(L.rgbid_default_ctx_set_interp_mode(O.INTERP_EXACT))
    try:
        a = host.keyframe_align(iD[0], grey[0], iD[1], grey[1], synth.TUM_K, host_driven=True)
        b = host.keyframe_align(iD[0], grey[0], iD[1], grey[1], synth.TUM_K, host_driven=False)
    finally:
        host.check(L.rgbid_default_ctx_set_interp_mode(O.INTERP_TEX8))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[1], tex8[1])
    again = host.keyframe_align(iD[0], grey[0], iD[1], grey[1], synth.TUM_K, host_driven=False)
    assert all(np.array_equal(x, y) for x, y in zip(again, tex8))


@pytest.mark.parametrize("rows,cols", [(120, 160), (480, 640)])
def test_keyframe_align_batched(rows, cols):
    """rgbid_kfalign_batched: N keyframe pairs with their own intrinsics and initial guesses in lock-step, no host round trip: every pair within the north-star
    tolerance of orc_keyframe_align, independent of its batch (a pair's result is the same bits whatever else rides along at a size where the launch plan
    does not change, and within rounding otherwise), host and device entry points identical."""
    import torch
    from rgbid import device, kfalign
    s = cols / 640.0
    K0 = (525.0 * s, 525.0 * s, (319.5 + 0.5) * s - 0.5, (239.5 + 0.5) * s - 0.5)
    n = 5
    iDa, ga, iDb, gb, Ks, Rgs, tgs = [], [], [], [], [], [], []
    for i in range(n):
        seq = synth.make_sequence(4, seed=synth.SEED + 31 * i, K=K0, rows=rows, cols=cols, device="cuda", trans_step=(0.008, 0.02), rot_step_deg=(0.3, 1.0))
        d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
        iD, grey, Rg, tg = _kf_pair(seq, d, c, 0, 2 + (i & 1))
        iDa.append(iD[0]); iDb.append(iD[1]); ga.append(grey[0]); gb.append(grey[1]); Ks.append(K0); Rgs.append(Rg); tgs.append(tg)
    iDa, iDb, ga, gb = [np.stack(x) for x in (iDa, iDb, ga, gb)]
    Ks = np.asarray(Ks, np.float32)
    # initial guesses: identity, and the ground truth perturbed (what a loop closer's PnP hands over)
    R0 = np.stack([np.eye(3) if i % 2 == 0 else Rgs[i] for i in range(n)]); t0 = np.stack([np.zeros(3) if i % 2 == 0 else tgs[i] + 0.004 for i in range(n)])
    ctx = device.Context(0)
    al = kfalign.KfAlign(ctx, rows, cols, n)
    R, t, cov = al.align(iDa, ga, iDb, gb, Ks, R0, t0)                                            # host entry point
    Rd, td, covd = al.align(*[torch.from_numpy(x).cuda() for x in (iDa, ga, iDb, gb)], Ks, R0, t0)   # device entry point
    assert np.array_equal(R, Rd) and np.array_equal(t, td) and np.array_equal(cov, covd)
    assert al.launches() == 4 + 6 + 4 + 1 + 13 * 7 + 1
    for i in range(n):
        Ro, to, covo = O.keyframe_align(iDa[i], ga[i], iDb[i], gb[i], K0, R0=R0[i], t0=t0[i])
        assert rot_angle(R[i], Ro) < 1e-4 and np.linalg.norm(t[i] - to) < 1e-4, (i, rot_angle(R[i], Ro), np.linalg.norm(t[i] - to))
        sc = np.sqrt(np.outer(np.diag(covo), np.diag(covo)))
        assert (np.abs(cov[i] - covo) / sc).max() < 1e-2
        assert rot_angle(R[i], Rgs[i]) < 4e-3 and np.linalg.norm(t[i] - tgs[i]) < 1.5e-2
        # the pair on its own
        R1, t1, c1 = al.align(iDa[i:i + 1], ga[i:i + 1], iDb[i:i + 1], gb[i:i + 1], Ks[i:i + 1], R0[i:i + 1], t0[i:i + 1])
        assert rot_angle(R1[0], R[i]) < 2e-6 and np.linalg.norm(t1[0] - t[i]) < 2e-6
    al.close(); ctx.close()


def test_keyframe_align_batched_partials_fit_every_pair_count_of_a_wide_geometry():
    """the aligner sized its partial-sum buffer for the 1-pair launch plan, assuming it has the most blocks per pair; the few-pair plans come from a
    schedule-length model, so at 2432x560 (tile rows not divisible by 3 or 4, more than 1 280 tiles) the 2-pair plan has MORE blocks per pair than the 1-pair plan and the
    normal-equation kernel wrote past the buffer.  The buffer now covers every pair count up to the capacity (and a plan that would not fit is refused): 1, 2 and 3 pairs
    of that geometry run, agree pairwise with the pairs aligned alone, and find the true motion."""
    import torch
    from rgbid import device, kfalign
    rows, cols = 560, 2432
    s = cols / 640.0
    K0 = (525.0 * s, 525.0 * s, (319.5 + 0.5) * s - 0.5, 279.5)
    n = 3
    iDa, ga, iDb, gb, Rgs, tgs = [], [], [], [], [], []
    for i in range(n):
        seq = synth.make_sequence(3, seed=synth.SEED + 77 * i, K=K0, rows=rows, cols=cols, device="cuda", trans_step=(0.008, 0.02), rot_step_deg=(0.3, 1.0))
        d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
        iD, grey, Rg, tg = _kf_pair(seq, d, c, 0, 2)
        iDa.append(iD[0]); iDb.append(iD[1]); ga.append(grey[0]); gb.append(grey[1]); Rgs.append(Rg); tgs.append(tg)
    iDa, iDb, ga, gb = [np.stack(x) for x in (iDa, iDb, ga, gb)]
    Ks = np.asarray([K0] * n, np.float32)
    R0 = np.stack([np.eye(3)] * n); t0 = np.zeros((n, 3))
    ctx = device.Context(0)
    al = kfalign.KfAlign(ctx, rows, cols, n)
    alone = [al.align(iDa[i:i + 1], ga[i:i + 1], iDb[i:i + 1], gb[i:i + 1], Ks[i:i + 1], R0[i:i + 1], t0[i:i + 1]) for i in range(n)]
    for m in (2, 3):
        R, t, cov = al.align(iDa[:m], ga[:m], iDb[:m], gb[:m], Ks[:m], R0[:m], t0[:m])
        for i in range(m):
            assert np.isfinite(R[i]).all() and np.isfinite(cov[i]).all()
            assert rot_angle(R[i], alone[i][0][0]) < 2e-6 and np.linalg.norm(t[i] - alone[i][1][0]) < 2e-6, (m, i)
            assert rot_angle(R[i], Rgs[i]) < 4e-3 and np.linalg.norm(t[i] - tgs[i]) < 1.5e-2, (m, i, rot_angle(R[i], Rgs[i]), np.linalg.norm(t[i] - tgs[i]))
    al.close(); ctx.close()


def test_keyframe_align_batched_many_pairs_one_wave_solve():
    """More pairs than compute units: the per-pair reduce-and-solve kernel runs as ONE wave per pair (kfalign.hip k_kfa_solve<64>: four slices of the fixed-order
    reduction per thread, the same doubles).  272 pairs carrying 4 distinct ones: duplicates agree to the last bit, and every pair agrees with its 4-pair run
    (256-thread workgroups; another launch plan of the normal equations) inside the tolerance (3e-5 here at 160x120, where a flipped nu bisection step moves a pose by ~1e-5; 1e-4 the bar),
    and with orc_keyframe_align inside the bar (1e-4 rad, 1e-4 m, 1e-2 on the covariance)."""
    from rgbid import device, kfalign
    rows, cols = 120, 160
    K0 = (131.25, 131.25, 79.875, 59.875)
    n, B = 4, 272
    iDa, ga, iDb, gb = [], [], [], []
    for i in range(n):
        seq = synth.make_sequence(4, seed=synth.SEED + 31 * i, K=K0, rows=rows, cols=cols, device="cuda", trans_step=(0.008, 0.02), rot_step_deg=(0.3, 1.0))
        d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
        iD, grey, _, _ = _kf_pair(seq, d, c, 0, 2 + (i & 1))
        iDa.append(iD[0]); iDb.append(iD[1]); ga.append(grey[0]); gb.append(grey[1])
    iDa, iDb, ga, gb = [np.stack(x) for x in (iDa, iDb, ga, gb)]
    idx = np.arange(B) % n
    Ks = np.tile(np.asarray(K0, np.float32), (B, 1))
    R0 = np.tile(np.eye(3), (B, 1, 1)); t0 = np.zeros((B, 3))
    ctx = device.Context(0)
    few = kfalign.KfAlign(ctx, rows, cols, n)
    Rf, tf, cf = few.align(iDa, ga, iDb, gb, Ks[:n], R0[:n], t0[:n])
    few.close()
    many = kfalign.KfAlign(ctx, rows, cols, B)
    R, t, cov = many.align(iDa[idx], ga[idx], iDb[idx], gb[idx], Ks, R0, t0)
    many.close(); ctx.close()
    for l in range(B):
        assert np.array_equal(R[l], R[l % n]) and np.array_equal(t[l], t[l % n]) and np.array_equal(cov[l], cov[l % n]), l
    for l in range(n):
        assert rot_angle(R[l], Rf[l]) < 3e-5 and np.linalg.norm(t[l] - tf[l]) < 3e-5, (l, rot_angle(R[l], Rf[l]), np.linalg.norm(t[l] - tf[l]))
    # and the one-wave solve is held to the oracle itself, not only to the other solve kernel
    for l in range(n):
        Ro, to, covo = O.keyframe_align(iDa[l], ga[l], iDb[l], gb[l], K0)
        sc = np.sqrt(np.outer(np.diag(covo), np.diag(covo)))
        dev = (rot_angle(R[l], Ro), np.linalg.norm(t[l] - to), (np.abs(cov[l] - covo) / sc).max())
        print(f"pair {l} of 272 against the oracle: {dev[0]:.2e} rad, {dev[1]:.2e} m, {dev[2]:.2e} covariance")
        assert np.isfinite(R[l]).all() and np.isfinite(t[l]).all() and np.isfinite(cov[l]).all()
        assert dev[0] < 1e-4 and dev[1] < 1e-4 and dev[2] < 1e-2, (l, dev)


def test_cli_eval_harness_on_tum_layout(tmp_path):
    """a TUM-layout dataset on disk (16-bit PNG depth x5000, 8-bit RGB PNG, association files) played through
    the `rgbid_slam_eval -eval` harness gives the oracle tracker's trajectory in the TUM trajectory format."""
    import os
    import subprocess
    from rgbid import tum, _lib
    n = 5
    seq = synth.make_sequence(n, device="cuda")
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    root = tmp_path / "synth_desk"
    os.makedirs(root / "depth"); os.makedirs(root / "rgb")
    hdr = "# line 1\n# line 2\n# timestamp filename\n"
    dl, cl = [], []
    for k in range(n):
        st = 1305031102.175304 + k / 30.0
        tum.write_png(str(root / "depth" / f"{st:.6f}.png"), (d[k].astype(np.uint32) * 5).astype(np.uint16))
        tum.write_png(str(root / "rgb" / f"{st:.6f}.png"), c[k])
        dl.append(f"{st:.6f} depth/{st:.6f}.png"); cl.append(f"{st:.6f} rgb/{st:.6f}.png")
    (root / "depth_associated.txt").write_text(hdr + "\n".join(dl) + "\n")
    (root / "rgb_associated.txt").write_text(hdr + "\n".join(cl) + "\n")
    exe = os.path.join(os.path.dirname(os.path.dirname(_lib.LIB_PATH)), "bin", "rgbid_slam_eval")
    out = subprocess.run([exe, "-eval", str(root) + "/", "-out", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    poses = np.loadtxt(tmp_path / "synth_desk_poses.txt")
    assert poses.shape == (n, 8)
    orc = O.Tracker(O.default_config())
    for k in range(n):
        orc.track(d[k], c[k])
    Rb, tb = orc.poses()
    lines = (tmp_path / "synth_desk_poses.txt").read_text().strip().split("\n")
    from scipy.spatial.transform import Rotation
    for k in range(n):
        assert lines[k].split(" ")[0] == "%.6f" % (1305031102.175304 + k / 30.0)
        assert np.linalg.norm(poses[k, 1:4] - tb[k]) < 1e-4
        assert rot_angle(Rotation.from_quat(poses[k, 4:]).as_matrix(), Rb[k]) < 1e-4
    misc = (tmp_path / "synth_desk_misc.txt").read_text().split("\n")
    assert misc[0].startswith("Mean time per frame: ") and misc[2].startswith("Max time per frame: ") and len(misc) >= 3 + n
    assert (tmp_path / "synth_desk_kf_times.txt").read_text().startswith("ObtainKeyframe ProcessKeyframeTotal Segmentation DescriptionBoW LoopDetection PoseGraphOptim\n")
    # the reference's two-thread playback (tracker thread woken through new_frame_cond_) writes the same trajectory
    os.makedirs(tmp_path / "thr")
    out = subprocess.run([exe, "-eval", str(root) + "/", "-out", str(tmp_path / "thr"), "-threaded"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert (tmp_path / "thr" / "synth_desk_poses.txt").read_text() == (tmp_path / "synth_desk_poses.txt").read_text()


def test_two_host_threads_share_the_library():
    """SURVEY 8(b) threading: the tracker thread and the KeyframeAlign thread of the reference call the bridge concurrently with no
    locking (per-thread streams).  Here: a VisodoTracker on one OS thread and KeyframeAlign calls on another, at the same time (ctypes
    drops the GIL inside the calls); both must give exactly what they give when run alone."""
    import threading
    n = 6
    seq = synth.make_sequence(n, K=SMALL_K, rows=120, cols=160, device="cuda", **SLOW)
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    big = synth.make_sequence(4, device="cuda", trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
    bd = big["depth"].cpu().numpy().astype(np.uint16); bc = big["rgb"].cpu().numpy()
    iD = [O.depth2invdepth(bd[k]) for k in (0, 3)]
    grey = [np.clip(np.rint(O.intensity(bc[k])), 0, 255).astype(np.uint8) for k in (0, 3)]
    kw = dict(rows=120, cols=160, fx=SMALL_K[0], fy=SMALL_K[1], cx=SMALL_K[2], cy=SMALL_K[3])

    def track_all():
        trk = host.Tracker(host.default_config(**kw))
        for k in range(n):
            trk.track(d[k], c[k])
        return trk.poses()

    def align_some(reps):
        return [host.keyframe_align(iD[0], grey[0], iD[1], grey[1], synth.TUM_K) for _ in range(reps)]

    ref_R, ref_t = track_all()
    ref_ka = align_some(1)[0]
    out = {}
    errs = []

    def run(name, fn, *a):
        try:
            out[name] = fn(*a)
        except Exception as e:  # pragma: no cover
            errs.append((name, e))

    th = [threading.Thread(target=run, args=("trk", track_all)), threading.Thread(target=run, args=("ka", align_some, 3))]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join()
    assert not errs, errs
    assert np.array_equal(out["trk"][0], ref_R) and np.array_equal(out["trk"][1], ref_t)
    for R, t, cov in out["ka"]:
        assert np.array_equal(R, ref_ka[0]) and np.array_equal(t, ref_ka[1]) and np.array_equal(cov, ref_ka[2])


def _blackout_sequence(n, black):
    seq = synth.make_sequence(n, K=SMALL_K, rows=120, cols=160, device="cuda", **SLOW)
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    for k in black:
        d[k][:] = 0                      # sensor drop-out: no valid depth -> empty normal equations -> NaN solve -> "I am LOST"
    return d, c


@both_modes
def test_cpp_tracker_lost_and_recovery(engine_backed):
    """visodo.cpp:2056-2113: a frame without valid depth makes the solve fail; the tracker declares itself lost, re-keys on the
    incoming frames (pushing no pose while it stays lost) and resumes odometry once a frame aligns again."""
    n = 8
    d, c = _blackout_sequence(n, black=(3,))
    kw = dict(rows=120, cols=160, fx=SMALL_K[0], fy=SMALL_K[1], cx=SMALL_K[2], cy=SMALL_K[3])
    trk = host.Tracker(host.default_config(**kw), engine_backed=engine_backed)
    orc = O.Tracker(O.default_config(**kw))
    rets = []
    for k in range(n):
        a, b = trk.track(d[k], c[k]), orc.track(d[k], c[k])
        assert a == b, k
        rets.append(b)
        if k:
            assert bool(trk.last_info().lost) == bool(orc.last_info().lost), k
    assert rets[3] is False and rets[4] is False and all(rets[5:])      # lost at 3, frame 4 cannot align to the empty keyframe, then recovers
    Ra, ta = trk.poses(); Rb, tb = orc.poses()
    assert len(Ra) == len(Rb) == n - 1                                   # the frame tracked while lost pushes no pose
    for k in range(len(Rb)):
        assert rot_angle(Ra[k], Rb[k]) < 1e-4 and np.linalg.norm(ta[k] - tb[k]) < 1e-4, k
    oa, ota, ca = trk.odometry(); ob, otb, cb = orc.odometry()
    assert len(oa) == len(ob)
    for k in range(len(ob)):
        assert rot_angle(oa[k], ob[k]) < 1e-4 and np.linalg.norm(ota[k] - otb[k]) < 1e-4
        assert np.allclose(ca[k], cb[k], rtol=1e-2, atol=1e-12 + 1e-2 * np.abs(cb[k]).max())


def test_track_dataset_tool_chunked(tmp_path):
    """BASELINE config 4 end to end on one GPU: a TUM-layout dataset on disk -> product dataset reader -> chunk-sharded engine ->
    TUM trajectory file.  With ONE chunk the file must equal the C++ tracker's trajectory (same frames, same algorithm); with several
    chunks the poses differ only at chunk heads (fresh keyframe, no velocity prior) by less than the documented 2e-3 rad / 5e-3 m."""
    import os
    import subprocess
    import sys
    from scipy.spatial.transform import Rotation
    from rgbid import tum
    n = 9
    seq = synth.make_sequence(n, device="cuda", trans_step=(0.004, 0.012), rot_step_deg=(0.2, 0.8))
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    root = tmp_path / "synth_office"
    os.makedirs(root / "depth"); os.makedirs(root / "rgb")
    lines = []
    for k in range(n):
        st = 1341847980.722988 + k / 30.0
        tum.write_png(str(root / "depth" / f"{st:.6f}.png"), (d[k].astype(np.uint32) * 5).astype(np.uint16))
        tum.write_png(str(root / "rgb" / f"{st:.6f}.png"), c[k])
        lines.append(f"{st:.6f} depth/{st:.6f}.png {st:.6f} rgb/{st:.6f}.png")
    (root / "assoc.txt").write_text("\n".join(lines) + "\n")
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "track_dataset.py")
    traj = {}
    for chunks in (1, 4):
        out = tmp_path / f"traj{chunks}.txt"
        r = subprocess.run([sys.executable, tool, str(root), "--match-file", "assoc.txt", "--chunks", str(chunks), "--out", str(out)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        traj[chunks] = np.loadtxt(out)
        assert traj[chunks].shape == (n, 8)
    orc = O.Tracker(O.default_config())
    for k in range(n):
        orc.track(d[k], c[k])
    Rb, tb = orc.poses()
    for k in range(n):
        assert np.linalg.norm(traj[1][k, 1:4] - tb[k]) < 1e-4 and rot_angle(Rotation.from_quat(traj[1][k, 4:]).as_matrix(), Rb[k]) < 1e-4
        assert np.linalg.norm(traj[4][k, 1:4] - tb[k]) < 5e-3 and rot_angle(Rotation.from_quat(traj[4][k, 4:]).as_matrix(), Rb[k]) < 2e-3
    # the same run with torch.distributed initialised on RCCL (one rank): the pose gather goes through all_gather_into_tensor on the GPU
    out = tmp_path / "traj4_dist.txt"
    r = subprocess.run([sys.executable, tool, str(root), "--match-file", "assoc.txt", "--chunks", "4", "--out", str(out), "--force-dist"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert out.read_text() == (tmp_path / "traj4.txt").read_text()


def test_cpp_bridge_and_containers(tmp_path):
    """tests/cpp/test_bridge.cpp: the reference's container semantics and bridge prototypes from plain C++ (g++, no HIP header),
    including the print-and-exit(0) error convention of pcl::gpu::error."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "rgbid-slam_amd", "lib")
    exe = str(tmp_path / "test_bridge")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "test_bridge.cpp"),
                           "-L" + lib, "-lrgbid_host", "-lrgbid_hip", "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all ok" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("\nok ") + r.stdout.startswith("ok ") >= 14
    r = subprocess.run([exe, "error"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Error: " in r.stdout and "internal.h:" in r.stdout and "FAILED" not in r.stdout, r.stdout + r.stderr


@both_modes
def test_cpp_objects_do_not_leak_device_memory(engine_backed):
    """VisodoTracker (with its engine in the engine-backed mode) and KeyframeAlign allocate dozens of ref-counted device arrays: 15 construct / use / destroy
    cycles return every byte"""
    import ctypes as C
    from rgbid import _lib
    L = _lib.lib()
    seq = synth.make_sequence(2, K=SMALL_K, rows=120, cols=160, device="cuda", **SLOW)
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    iD = [O.depth2invdepth(np.zeros((480, 640), np.uint16) + 1500) for _ in range(2)]
    grey = [np.full((480, 640), 100, np.uint8) for _ in range(2)]
    kw = dict(rows=120, cols=160, fx=SMALL_K[0], fy=SMALL_K[1], cx=SMALL_K[2], cy=SMALL_K[3])

    def free_bytes():
        f, t = C.c_size_t(), C.c_size_t()
        assert L.rgbid_mem_info(C.byref(f), C.byref(t)) == 0
        return f.value

    def cycle():
        trk = host.Tracker(host.default_config(**kw), engine_backed=engine_backed)
        trk.track(d[0], c[0]); trk.track(d[1], c[1])
        trk.close()
        host.keyframe_align(iD[0], grey[0], iD[1], grey[1], synth.TUM_K)

    cycle()
    torch_free = free_bytes()
    for _ in range(15):
        cycle()
    assert abs(free_bytes() - torch_free) < (8 << 20), (torch_free, free_bytes())


@both_modes
def test_cpp_tracker_load_settings_and_calibration_files(tmp_path, engine_backed):
    """VisodoTracker::loadSettings ([VISODO] keys of config_data/visodoRGBDconfig.ini) and loadCalibration ([CALIBRATION]) switch the
    tracker exactly like the equivalent constructor arguments: trajectory = oracle with that configuration."""
    (tmp_path / "visodo.ini").write_text("[VISODO]\nM_ESTIMATOR = Huber\nMOTION_MODEL = none\nWARP_ORDER = warpFirst\nIMAGE_FILTERING = gradients\n"
                                         "SIGMA_ESTIMATOR = sigmaConst\nINTEGRATION_VISRATIO_THRESHOLD = 0.93\nODOMETRY_VISRATIO_THRESHOLD = 0.97\nFINEST_PYR_LEVEL = 1\n")
    K = (SMALL_K[0] * 1.02, SMALL_K[1] * 0.98, SMALL_K[2] + 0.7, SMALL_K[3] - 0.4)
    (tmp_path / "calib.ini").write_text(f"[CALIBRATION]\nfx = {K[0]}\nfy = {K[1]}\ncx = {K[2]}\ncy = {K[3]}\nkd = 0 0 0 0 0\nfactor_depth = 0.96\n")
    n = 5
    seq = synth.make_sequence(n, K=K, rows=120, cols=160, device="cuda", **SLOW)
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    trk = host.Tracker(host.default_config(rows=120, cols=160))         # defaults, everything else comes from the two files
    trk.load_settings(str(tmp_path / "visodo.ini"))
    trk.load_calibration(str(tmp_path / "calib.ini"))
    if engine_backed:
        trk.set_engine_backed(True)        # after the files: the engine is created from what they set (Huber, no motion model, warp-first, filtered gradients, ...)
    orc = O.Tracker(O.default_config(rows=120, cols=160, fx=K[0], fy=K[1], cx=K[2], cy=K[3], factor_depth=0.96, mestimator=O.HUBER, motion_model=O.NO_MM,
                                     warping=O.WARP_FIRST, image_filtering=O.FILTER_GRADS, sigma_estimator=O.SIGMA_CONS, visratio_integr=0.93,
                                     visratio_odo=0.97, finest_level=1))
    for k in range(n):
        assert trk.track(d[k], c[k]) == orc.track(d[k], c[k])
        if k:
            ia, ib = trk.last_info(), orc.last_info()
            assert bool(ia.odo_kf_switched) == bool(ib.odo_kf_switched) and bool(ia.integr_kf_switched) == bool(ib.integr_kf_switched)
    Ra, ta = trk.poses(); Rb, tb = orc.poses()
    for k in range(n):
        assert rot_angle(Ra[k], Rb[k]) < 1e-4 and np.linalg.norm(ta[k] - tb[k]) < 1e-4, k


def _cmp_backend_streams(trk, orc, rows, cols, K=None, pose_tol=1e-4):
    K = K or SMALL_K
    """Pose / PoseConstraint / keyframe streams of the product (collecting TrackerSink through the C-ABI) against the oracle's."""
    ia, Ra, ta = trk.sink_poses(); ib, Rb, tb = orc.sink_poses()
    assert np.array_equal(ia, ib)
    for k in range(len(ib)):
        assert rot_angle(Ra[k], Rb[k]) < pose_tol and np.linalg.norm(ta[k] - tb[k]) < pose_tol, k
    ca, cb = trk.constraints(), orc.constraints()
    assert [(c["ini"], c["end"], c["type"]) for c in ca] == [(c["ini"], c["end"], c["type"]) for c in cb]
    for a, b in zip(ca, cb):
        assert rot_angle(a["R"], b["R"]) < pose_tol and np.linalg.norm(a["t"] - b["t"]) < pose_tol, (b["ini"], b["end"], b["type"])
        sc = np.sqrt(np.outer(np.diag(b["cov"]), np.diag(b["cov"]))) + 1e-30
        assert (np.abs(a["cov"] - b["cov"]) / sc).max() < 1e-2, (b["ini"], b["end"], b["type"])
    assert trk.num_keyframes() == orc.num_keyframes()
    for i in range(orc.num_keyframes()):
        a, b = trk.peek_keyframe(i), orc.keyframe(i)
        assert a["id"] == b["id"]
        assert rot_angle(a["R"], b["R"]) < pose_tol and np.linalg.norm(a["t"] - b["t"]) < pose_tol
        assert rot_angle(a["R_rel"], b["R_rel"]) < pose_tol and np.linalg.norm(a["t_rel"] - b["t_rel"]) < pose_tol
        assert np.array_equal(a["colors"], b["colors"])                                   # bytes: exact
        assert np.count_nonzero(a["overlap_mask"] != b["overlap_mask"]) <= 2e-3 * rows * cols   # pixels at the 0.020 covisibility gate may flip
        da, db = a["depthinv"], b["depthinv"]
        assert np.count_nonzero(np.isnan(da) != np.isnan(db)) <= 2e-3 * db.size
        m = ~np.isnan(da) & ~np.isnan(db)
        rel = np.abs(da[m] - db[m]) / db[m]
        assert np.count_nonzero(rel > 1e-4) <= max(16, 5e-3 * rel.size) and np.median(rel) < 1e-5
        # normals (planes 1,2 are only written where plane 0 is valid, maps.cu:171-176).  They amplify differences of the fused map by
        # f/w (~260x here), so (1) they must be EXACTLY the normal map of the exported inverse depth (oracle function on the product's map,
        # a few ulp), and (2) agree with the oracle tracker's normals in angle on all but a few percent of the pixels.
        na, nb = a["normals"], b["normals"]
        va, vb = ~np.isnan(na[0]), ~np.isnan(nb[0])
        assert np.count_nonzero(va != vb) <= 6e-3 * vb.size
        gx, gy = O.gradient(da)
        own = O.nmap_gradients(da, gx, gy, K).reshape(3, rows, cols)
        vo = ~np.isnan(own[0])
        assert np.count_nonzero(vo != va) <= 4                                             # the 0.1 viewing-angle gate
        assert np.abs(own[:, vo & va] - na[:, vo & va]).max() < 2e-6
        both = va & vb
        ang = np.arccos(np.clip((na[:, both] * nb[:, both]).sum(0), -1, 1))
        assert np.count_nonzero(ang > 0.05) <= 0.03 * both.sum() and np.median(ang) < 5e-3, (np.median(ang), np.mean(ang > 0.05))
    return len(cb), orc.num_keyframes()


@both_modes
def test_backend_streams_keyframe_switches(engine_backed):
    """what trackNewFrame hands to the back-end (visodo.cpp:1612-1652, 2033-2038, 2155-2164) -- one Pose per frame, one
    SEQ_ODO PoseConstraint per tracked frame, and at each integration-keyframe switch the exported keyframe (global + relative pose,
    overlap mask, colours, fused inverse depth, normals) plus its SEQ_KF constraint -- equals the oracle's on a sequence that switches."""
    rows, cols, n = 120, 160, 9
    seq = synth.make_sequence(n, K=SMALL_K, rows=rows, cols=cols, device="cuda", trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    kw = dict(rows=rows, cols=cols, fx=SMALL_K[0], fy=SMALL_K[1], cx=SMALL_K[2], cy=SMALL_K[3], visratio_odo=0.985, visratio_integr=0.97)
    trk = host.Tracker(host.default_config(**kw), engine_backed=engine_backed); trk.collect()
    orc = O.Tracker(O.default_config(**kw))
    for k in range(n):
        assert trk.track(d[k], c[k]) == orc.track(d[k], c[k])
        if k:
            ia, ib = trk.last_info(), orc.last_info()
            assert bool(ia.integr_kf_switched) == bool(ib.integr_kf_switched) and bool(ia.odo_kf_switched) == bool(ib.odo_kf_switched), k
    n_c, n_kf = _cmp_backend_streams(trk, orc, rows, cols)
    assert n_kf >= 2 and n_c == (n - 1) + n_kf                 # every switch exported a keyframe and its SEQ_KF constraint
    info = trk.peek_keyframe(0)
    assert np.allclose(info["K"], [[SMALL_K[0], 0, SMALL_K[2]], [0, SMALL_K[1], SMALL_K[3]], [0, 0, 1]]) and not info["kd"].any()
    assert info["id"] == 0 and np.allclose(info["R"], np.eye(3)) and not info["t"].any()
    # the consumer side of the bounded buffer
    assert trk.pop_keyframe() and trk.num_keyframes() == n_kf - 1 and trk.peek_keyframe(0)["id"] == orc.keyframe(1)["id"]
    trk.close(); orc.close()


@both_modes
def test_backend_streams_lost_frame_and_full_buffer(engine_backed):
    """visodo.cpp:2066-2085: the frame that loses tracking pushes a dummy SEQ_ODO constraint (identity, covariance 100 I), a pose that repeats
    the back-end's last one, and -- through resetIntegrationKeyframe -- the keyframe before the failure with its SEQ_KF constraint.
    With a full keyframe buffer (try_push fails, :1644) the keyframe AND its constraint are dropped."""
    n = 8
    d, c = _blackout_sequence(n, black=(3,))
    kw = dict(rows=120, cols=160, fx=SMALL_K[0], fy=SMALL_K[1], cx=SMALL_K[2], cy=SMALL_K[3])
    trk = host.Tracker(host.default_config(**kw), engine_backed=engine_backed); trk.collect()
    full = host.Tracker(host.default_config(**kw), engine_backed=engine_backed); full.collect(keyframe_capacity=1)
    orc = O.Tracker(O.default_config(**kw))
    for k in range(n):
        r = orc.track(d[k], c[k])
        assert trk.track(d[k], c[k]) == r and full.track(d[k], c[k]) == r
    _cmp_backend_streams(trk, orc, 120, 160)
    cons = orc.constraints()
    dummy = [q for q in cons if q["type"] == O.SEQ_ODO and q["end"] == 3][0]
    assert np.array_equal(dummy["R"], np.eye(3)) and not dummy["t"].any() and np.array_equal(dummy["cov"], 100 * np.eye(6))
    ids, Rs, ts = trk.sink_poses()
    assert np.array_equal(Rs[3], Rs[2]) and np.array_equal(ts[3], ts[2])
    # bounded buffer: only the first keyframe fits; later switches push neither keyframe nor SEQ_KF constraint
    assert full.num_keyframes() == 1
    kf_full = [q for q in full.constraints() if q["type"] == host.SEQ_KF]
    kf_all = [q for q in trk.constraints() if q["type"] == host.SEQ_KF]
    assert len(kf_full) == 1 and len(kf_all) == trk.num_keyframes() >= 1
    assert len([q for q in full.constraints() if q["type"] == host.SEQ_ODO]) == len([q for q in cons if q["type"] == O.SEQ_ODO])
    trk.close(); full.close(); orc.close()


@both_modes
def test_backend_pose_moved_by_optimiser_is_continued(engine_backed):
    """visodo.cpp:2161-2162: the pose pushed for frame k continues poses_.back() AS THE BACK-END HOLDS IT (a pose-graph optimisation may
    have moved it), composed with the sequential odometry -- not the tracker's own global estimate."""
    n = 5
    seq = synth.make_sequence(n, K=SMALL_K, rows=120, cols=160, device="cuda", **SLOW)
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    kw = dict(rows=120, cols=160, fx=SMALL_K[0], fy=SMALL_K[1], cx=SMALL_K[2], cy=SMALL_K[3])
    trk = host.Tracker(host.default_config(**kw), engine_backed=engine_backed); trk.collect()
    for k in range(3):
        trk.track(d[k], c[k])
    Rm = host.expmap_rot([0.02, -0.01, 0.03]); tm = np.array([0.5, -0.25, 1.0])
    trk.set_sink_pose(2, Rm, tm)
    trk.track(d[3], c[3])
    ids, Rs, ts = trk.sink_poses()
    q = trk.constraints()[-1]
    assert (q["ini"], q["end"], q["type"]) == (2, 3, host.SEQ_ODO)
    assert np.allclose(Rs[3], Rm @ q["R"], atol=1e-12) and np.allclose(ts[3], tm + Rm @ q["t"], atol=1e-12)
    Rg, tg = trk.poses()                                   # the tracker's own trajectory is untouched
    assert rot_angle(Rg[3], Rs[3]) > 1e-2
    trk.close()


def test_async_bridge_changes_nothing_but_the_time():
    """include/rgbid/containers.hpp ScopedAsyncBridge: trackNewFrame runs its device calls without the per-call timing events and stream
    synchronisations of the reference's bridge contract (it ignores the returned milliseconds).  Program order on the per-thread stream is
    unchanged, so every pose, covariance and fused map must be BIT-identical to the fully synchronous run."""
    n = 7
    seq = synth.make_sequence(n, K=SMALL_K, rows=120, cols=160, device="cuda", trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    kw = dict(rows=120, cols=160, fx=SMALL_K[0], fy=SMALL_K[1], cx=SMALL_K[2], cy=SMALL_K[3], visratio_odo=0.985, visratio_integr=0.97)
    out = []
    for on in (0, 1):
        trk = host.Tracker(host.default_config(**kw), engine_backed=False); trk.set_async_bridge(on); trk.collect()
        for k in range(n):
            trk.track(d[k], c[k])
        R, t = trk.poses(); oR, ot, ocov = trk.odometry(); kd, kw_ = trk.keyframe_maps()
        nrm = trk.peek_keyframe(0)["normals"]
        nrm[:, np.isnan(nrm[0])] = np.nan          # planes 1, 2 of an invalid normal are untouched (uninitialised) memory, as in the reference
        out.append((R, t, ocov, kd, kw_, trk.num_keyframes(), nrm))
        trk.close()
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_engine_backed_tracker_equals_host_driven_tracker():
    """VisodoTracker::setEngineBacked(true): the frame runs as one step of a one-lane engine in the bit-exact numerics class.  Both modes run the
    same kernels on the same data in the same order, so everything the application and the back-end see -- return values, poses, odometry
    constraints and covariances, keyframe decisions, exported keyframes, fused maps, lastInfo -- must be IDENTICAL, bit for bit, on a sequence
    that switches keyframes, loses tracking and recovers."""
    n = 12
    seq = synth.make_sequence(n, K=SMALL_K, rows=120, cols=160, device="cuda", trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    d[7][:] = 0
    kw = dict(rows=120, cols=160, fx=SMALL_K[0], fy=SMALL_K[1], cx=SMALL_K[2], cy=SMALL_K[3], visratio_odo=0.985, visratio_integr=0.97)
    out = []
    for eb in (False, True):
        trk = host.Tracker(host.default_config(**kw), engine_backed=eb); trk.collect()
        rets, infos = [], []
        for k in range(n):
            rets.append(trk.track(d[k], c[k]))
            i = trk.last_info()
            infos.append((i.lost, i.odo_kf_switched, i.integr_kf_switched, i.visratio_odo, i.visratio_integr, i.sigma_int, i.sigma_depthinv, i.nu_int, i.nu_depthinv))
        R, t = trk.poses(); oR, ot, ocov = trk.odometry(); kd, kw_ = trk.keyframe_maps(); cd, ci = trk.current_maps()
        ids, sR, st = trk.sink_poses()
        cons = [(q["ini"], q["end"], q["type"], q["R"], q["t"], q["cov"]) for q in trk.constraints()]
        kfs = []
        for i in range(trk.num_keyframes()):
            q = trk.peek_keyframe(i)
            nrm = q["normals"]; nrm[:, np.isnan(nrm[0])] = np.nan
            kfs.append((q["id"], q["R"], q["t"], q["R_rel"], q["t_rel"], q["K"], q["kd"], q["overlap_mask"], q["colors"], q["depthinv"], nrm))
        out.append(dict(rets=rets, infos=np.array(infos, dtype=np.float64), R=R, t=t, oR=oR, ot=ot, ocov=ocov, kd=kd, kw=kw_, cd=cd, ci=ci, ids=ids, sR=sR, st=st, cons=cons, kfs=kfs))
        trk.close()
    a, b = out
    assert a["rets"] == b["rets"] and not a["rets"][7] and sum(a["rets"]) >= 8
    assert len(a["kfs"]) == len(b["kfs"]) >= 2 and len(a["cons"]) == len(b["cons"])
    for key in ("infos", "R", "t", "oR", "ot", "ocov", "kd", "kw", "cd", "ci", "ids", "sR", "st"):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key
    for qa, qb in zip(a["cons"], b["cons"]):
        assert qa[:3] == qb[:3] and all(np.array_equal(x, y) for x, y in zip(qa[3:], qb[3:])), qa[:3]
    for qa, qb in zip(a["kfs"], b["kfs"]):
        assert qa[0] == qb[0] and all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(qa[1:], qb[1:])), qa[0]


def test_engine_backed_is_the_default_and_the_mode_is_settled_at_the_first_frame(capfd):
    """Round 5: an unchanged caller gets the device-resident engine; what the engine cannot take over falls back to the host-driven loop by itself (logged),
    decided at the first frame with the configuration as it is THEN (a calibration loaded after setEngineBacked must not be ignored); the mode
    cannot change once a frame has been taken."""
    import os
    kw = dict(rows=120, cols=160, fx=SMALL_K[0], fy=SMALL_K[1], cx=SMALL_K[2], cy=SMALL_K[3])
    seq = synth.make_sequence(2, K=SMALL_K, rows=120, cols=160, device="cuda", **SLOW)
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    trk = host.Tracker(host.default_config(**kw))
    assert trk.engine_backed()
    trk.track(d[0], c[0])
    assert trk.engine_backed()
    with pytest.raises(Exception):
        trk.set_engine_backed(False)           # only before the first frame
    trk.close()
    # CHI_SQUARED termination is an engine configuration now
    trk = host.Tracker(host.default_config(termination=O.CHI_SQUARED, **kw)); trk.set_engine_backed(True); trk.track(d[0], c[0]); assert trk.engine_backed(); trk.close()
    # an obstacle (here: the environment override) -> explicit request refused, default falls back with one line on stderr
    os.environ["RGBID_VISODO_HOST_DRIVEN"] = "1"
    try:
        trk = host.Tracker(host.default_config(**kw))
        with pytest.raises(Exception):
            trk.set_engine_backed(True)
        capfd.readouterr()
        trk.track(d[0], c[0])
        assert not trk.engine_backed() and "host-driven frame loop" in capfd.readouterr().err
        trk.close()
    finally:
        del os.environ["RGBID_VISODO_HOST_DRIVEN"]


@pytest.mark.parametrize("case", ["chi_squared_warp_first", "chi_squared_pyr_first", "custom_calibration"])
def test_engine_backed_equals_host_driven_in_the_round5_configurations(case, tmp_path):
    """The two configurations that were host-driven only until round 4 -- CHI_SQUARED termination (visodo.cpp:1134-1164) and the custom-calibration front-end
    (prepareImagesCustomCalibration, :775-824) -- through the engine: poses, covariances, lastInfo, current and fused maps IDENTICAL to the host-driven loop."""
    n = 6
    full = case == "custom_calibration"
    rows, cols, K = (480, 640, synth.TUM_K) if full else (120, 160, SMALL_K)
    seq = synth.make_sequence(n, K=K, rows=rows, cols=cols, device="cuda", **SLOW)
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    kw = dict(rows=rows, cols=cols, fx=K[0], fy=K[1], cx=K[2], cy=K[3])
    if not full:
        kw.update(warping=O.WARP_FIRST if case == "chi_squared_warp_first" else O.PYR_FIRST, termination=O.CHI_SQUARED)
    out = []
    for eb in (False, True):
        trk = host.Tracker(host.default_config(**kw), engine_backed=eb)
        if full:
            from tests.test_gpu_calib import CALIB_INI
            (tmp_path / "calib.ini").write_text(CALIB_INI)
            trk.load_calibration(str(tmp_path / "calib.ini"))
        rets, infos, maps = [], [], []
        for k in range(n):
            rets.append(trk.track(d[k], c[k]))
            i = trk.last_info()
            infos.append((i.lost, i.odo_kf_switched, i.integr_kf_switched, i.visratio_odo, i.visratio_integr, i.sigma_int, i.sigma_depthinv, i.nu_int, i.nu_depthinv))
            maps.append(trk.current_maps())
        assert trk.engine_backed() == eb
        R, t = trk.poses(); oR, ot, ocov = trk.odometry(); kd, kw_ = trk.keyframe_maps()
        out.append(dict(rets=rets, infos=np.array(infos, dtype=np.float64), R=R, t=t, oR=oR, ot=ot, ocov=ocov, kd=kd, kw=kw_,
                        cd=np.stack([m[0] for m in maps]), ci=np.stack([m[1] for m in maps])))
        trk.close()
    a, b = out
    assert a["rets"] == b["rets"] and sum(a["rets"]) == n - 1
    for key in ("infos", "R", "t", "oR", "ot", "ocov", "kd", "kw", "cd", "ci"):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key
    if full:
        assert np.isfinite(a["cd"][-1]).mean() > 0.6


def test_tracker_preview_is_the_same_in_both_modes():
    """What the application's viewer reads with the preview on (scene_view_ / intensity_view_ / depthinv_view_, getImage visodo.cpp:559-580, 2237-2241) through
    rgbid_tracker_scene_view: the host-driven tracker shades with generateImageRGB, the engine-backed one takes the engine's preview -- the same kernel on the same
    maps with the same light: bit-identical after every tracked frame of a sequence that switches its integration keyframe."""
    n = 7
    seq = synth.make_sequence(n, K=SMALL_K, rows=120, cols=160, device="cuda", trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    kw = dict(rows=120, cols=160, fx=SMALL_K[0], fy=SMALL_K[1], cx=SMALL_K[2], cy=SMALL_K[3], visratio_integr=0.97, preview=1)
    views = []
    for eb in (False, True):
        trk = host.Tracker(host.default_config(**kw), engine_backed=eb)
        out = []
        for k in range(n):
            if trk.track(d[k], c[k]):
                rgb, inten, dinv, changed = trk.scene_view()
                assert changed
                out.append((k, rgb, inten, dinv, bool(trk.last_info().integr_kf_switched)))
        views.append(out)
        trk.close()
    a, b = views
    assert len(a) == len(b) >= n - 2 and any(v[4] for v in a)
    for va, vb in zip(a, b):
        assert va[0] == vb[0] and va[4] == vb[4]
        assert np.array_equal(va[1], vb[1]), va[0]
        assert np.array_equal(va[2], vb[2], equal_nan=True) and np.array_equal(va[3], vb[3], equal_nan=True), va[0]
    assert a[-1][1].any()                                            # something was shaded


@both_modes
def test_tracker_reset_starts_over(engine_backed):
    """VisodoTracker::reset (src/visodo.cpp:519-553): the next frame is a first frame again -- the same frames tracked after a reset give the same poses, bit for
    bit, as the first pass (in the engine-backed mode the one-lane engine starts over with it)"""
    n = 5
    seq = synth.make_sequence(n, K=SMALL_K, rows=120, cols=160, device="cuda", trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    kw = dict(rows=120, cols=160, fx=SMALL_K[0], fy=SMALL_K[1], cx=SMALL_K[2], cy=SMALL_K[3])
    trk = host.Tracker(host.default_config(**kw), engine_backed=engine_backed)
    passes = []
    for rep in range(2):
        rets = [trk.track(d[k], c[k]) for k in range(n)]
        R, t = trk.poses()
        passes.append((rets, R.copy(), t.copy()))
        trk.reset()
    assert passes[0][0] == passes[1][0] and passes[0][0][0] is False and all(passes[0][0][1:])
    assert np.array_equal(passes[0][1], passes[1][1]) and np.array_equal(passes[0][2], passes[1][2])
    trk.close()


def test_engine_backed_tracker_outlives_the_thread_that_fed_it():
    """The reference runs trackNewFrame on a thread of its own and destroys the tracker from the main thread afterwards.  The engine of the engine-backed mode
    therefore lives on a context the TRACKER owns (the per-thread default context of containers.hpp ends with its thread): frames tracked on a worker thread,
    results read and the tracker destroyed on the main thread after the worker has exited."""
    import threading
    n = 5
    seq = synth.make_sequence(n, K=SMALL_K, rows=120, cols=160, device="cuda", **SLOW)
    d = seq["depth"].cpu().numpy().astype(np.uint16); c = seq["rgb"].cpu().numpy()
    kw = dict(rows=120, cols=160, fx=SMALL_K[0], fy=SMALL_K[1], cx=SMALL_K[2], cy=SMALL_K[3])
    ref = host.Tracker(host.default_config(**kw), engine_backed=True)
    for k in range(n):
        ref.track(d[k], c[k])
    Rr, tr = ref.poses(); kdr, kwr = ref.keyframe_maps()
    ref.close()
    trk = host.Tracker(host.default_config(**kw), engine_backed=True)
    errs = []

    def work():
        try:
            for k in range(n):
                trk.track(d[k], c[k])
        except Exception as e:  # pragma: no cover
            errs.append(e)

    th = threading.Thread(target=work); th.start(); th.join()
    assert not errs, errs
    R, t = trk.poses(); kd, kw_ = trk.keyframe_maps()          # main thread, after the worker (and its thread-local context) are gone
    assert np.array_equal(R, Rr) and np.array_equal(t, tr) and np.array_equal(kd, kdr, equal_nan=True) and np.array_equal(kw_, kwr, equal_nan=True)
    trk.track(d[n - 1], c[n - 1])                              # and it keeps tracking from here
    trk.close()
