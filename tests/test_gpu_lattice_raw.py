"""The level-0 residual lattice gathered from the raw input frame (u16 depth + rgb24, converted in registers) against the same lattice gathered from the
fp32 maps that frame preparation converts the frame into.  Everything here is BIT identity -- the raw source changes which bytes are loaded, not a value:

  1. the conversion (warp_device.h frame_px, through the accessors the lattice uses) equals launch_prep_frame for all 65 536 depths and all 2^24 colours;
  2. the kernel's residual arrays equal the fp32 variant's byte for byte, masked lane included;
  3. an engine run is byte-identical (records, keyframe maps, exported keyframes) with the raw source on (default) and off (RGBID_ENGINE_LATTICE_RAW=0).

Lattice strides: a 120 x 160 frame gives stride 4 (1 000 samples asked) and stride 2 (4 000).  A 122 x 166 frame cannot be halved twice (61 rows), so its
lattice has stride 2 or 1 whatever is asked; both are run.  Its 166 columns also put it outside the FAST class (rows of whole 4-pixel groups), so it runs the
EXACT class, whose four single-texel taps go through the byte loads of the raw source.
"""
import os

import numpy as np
import pytest
import torch

from rgbid import batched as BT
from rgbid import device
from rgbid import engine as E
from rgbid._lib import RgbidError
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bt(ctx):
    return BT.Batched(ctx)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def prep(bt, depth, rgb, factor):
    lanes, rows, cols = depth.shape
    outs = [torch.zeros((lanes, rows, cols), device="cuda") for _ in range(5)]
    bt.prep_frame(depth, rgb, *outs, factor)
    return outs[0], outs[1]


# ---- 1. the conversion ---------------------------------------------------------------------------------------------------------------------
def test_conversion_exhaustive(bt):
    """one 4096 x 4096 single-lane image holds every colour once and every depth 256 times: point sample, tap-pair load and single-texel tap of the raw
    source must equal launch_prep_frame's maps bit for bit"""
    n = 4096
    idx = torch.arange(n * n, device="cuda", dtype=torch.int64).view(1, n, n)
    rgb = torch.stack([idx & 255, (idx >> 8) & 255, (idx >> 16) & 255], -1).to(torch.uint8).contiguous()
    d16 = idx & 65535
    depth = (d16 - 65536 * (d16 >= 32768)).to(torch.int16).contiguous()   # the u16 bit patterns 0 .. 65535
    assert int(depth.view(-1)[65535].item()) == -1
    iD, I = prep(bt, depth, rgb, 1.0)
    got = [torch.full((1, n, n), 7.0, device="cuda") for _ in range(3)]
    bt.frame_px(depth, rgb, *got, 1.0)
    assert same_bits(got[0], iD), "inverse depth"
    assert same_bits(got[1], I), "intensity, tap pair"
    assert same_bits(got[2], I), "intensity, single texel"
    assert torch.isnan(iD.view(-1)[0]) and float(iD.view(-1)[65535]) == float(iD.view(-1)[10000])   # depth 0 invalid, 65 535 clamped to 10 m


@pytest.mark.parametrize("rows,cols,lanes", [(256, 256, 1), (122, 166, 3), (8, 5, 2), (2, 2, 1)])
@pytest.mark.parametrize("factor", [0.96, 5.0])
def test_conversion_other_factors_and_odd_geometry(bt, rows, cols, lanes, factor):
    """every depth under other depth factors; rgb rows that are no multiple of 4 bytes (166 / 5 / 2 columns: the 12-byte window starts at every offset of
    a dword, and is moved back at the end of the image)"""
    r = util.rng(311 + rows)
    d = r.integers(0, 65536, (lanes, rows, cols)).astype(np.uint16)
    if rows * cols == 65536:
        d[0] = np.arange(65536, dtype=np.uint16).reshape(rows, cols)
    c = r.integers(0, 256, (lanes, rows, cols, 3)).astype(np.uint8)
    depth, rgb = torch.from_numpy(d.view(np.int16)).cuda(), torch.from_numpy(c).cuda()
    iD, I = prep(bt, depth, rgb, factor)
    got = [torch.full((lanes, rows, cols), 7.0, device="cuda") for _ in range(3)]
    bt.frame_px(depth, rgb, *got, factor)
    assert same_bits(got[0], iD) and same_bits(got[1], I) and same_bits(got[2], I)


def test_raw_source_refuses_a_frame_off_its_boundaries(bt):
    """an rgb image that does not start on a 4-byte boundary is an error of the call, never a silent switch to the other source"""
    rows, cols = 8, 8
    big = torch.zeros(rows * cols * 3 + 4, dtype=torch.uint8, device="cuda")
    rgb = big[1:1 + rows * cols * 3].view(1, rows, cols, 3)
    depth = torch.zeros((1, rows, cols), dtype=torch.int16, device="cuda")
    outs = [torch.zeros((1, rows, cols), device="cuda") for _ in range(3)]
    with pytest.raises(RgbidError):
        bt.frame_px(depth, rgb, *outs, 1.0)


# ---- 2. the kernel ---------------------------------------------------------------------------------------------------------------------------
def K_for(cols):
    s = cols / 640.0
    return (525.0 * s, 525.0 * s, 319.5 * s, 239.5 * s)


def make_frame(rows, cols, lanes, seed):
    """a smooth scene 0.8 .. 3 m deep with texture: zeros, values above 10 000, 65 535, a fully invalid row, saturated colours"""
    ds, cs = [], []
    v, u = np.mgrid[0:rows, 0:cols].astype(np.float64)
    for l in range(lanes):
        r = util.rng(seed + l)
        z = 1800 + 700 * np.sin(u / (cols / 5.0) + l) * np.cos(v / (rows / 3.0)) + 300 * (u / cols) + 15 * r.standard_normal((rows, cols))
        d = np.clip(z, 500, 9000).astype(np.uint16)
        d[r.random((rows, cols)) < 0.05] = 0
        d[rows // 3, :] = 0                                   # a fully invalid row
        d[5:9, 7:19] = 12000                                  # beyond the 10 m clamp
        d[10, 3:40] = 65535
        d[rows - 1, cols - 1] = 65535
        d[0, 0] = 10001
        tex = 127 + 60 * np.sin(u / 7.0) * np.cos(v / 5.0) + 40 * np.sin((u + 2 * v) / 13.0)
        c = np.stack([tex + 8 * r.standard_normal((rows, cols)) + 20 * k for k in (-1, 0, 1)], -1)
        c = np.clip(c, 0, 255).astype(np.uint8)
        c[20:30, 30:50] = 255                                 # saturated
        c[40:44, 60:90] = 0
        c[rows - 1, cols - 2:] = (255, 0, 255)
        ds.append(d); cs.append(c)
    return torch.from_numpy(np.stack(ds).view(np.int16)).cuda(), torch.from_numpy(np.stack(cs)).cuda()


def warps(K, lanes, kind):
    Rs, ts = [], []
    for l in range(lanes):
        if kind == "identity":
            R, t = np.eye(3), np.zeros(3)
        elif kind == "motion":
            R, t = util.small_motion(util.rng(77 + l), K, 0.015, 0.8)[:2]
        else:   # a rotation that sends a large part of the lattice across the image border (and a roll, so that both axes leave)
            a, b = np.deg2rad(22.0 + 3 * l), np.deg2rad(6.0)
            Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
            Rz = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
            R, t = Ry @ Rz, np.array([0.02, -0.01, 0.03])
        Rp, tp = util.project(K, *util.inv_pose(R, t))
        Rs.append(Rp); ts.append(tp)
    return Rs, ts


@pytest.fixture(scope="module")
def kernel_cases(bt):
    """per geometry: the raw current frame, its prepared fp32 maps, and a keyframe prepared from a second frame of the same scene"""
    out = {}
    for rows, cols in ((120, 160), (122, 166)):
        depth, rgb = make_frame(rows, cols, 3, 500)
        kdepth, krgb = make_frame(rows, cols, 3, 900)
        Wc, Ic = prep(bt, depth, rgb, 1.0)
        W0, I0 = prep(bt, kdepth, krgb, 1.0)
        out[(rows, cols)] = dict(depth=depth, rgb=rgb, Wc=Wc, Ic=Ic, W0=W0, I0=I0)
    return out


@pytest.mark.parametrize("rows,cols,ns,stride,fast", [(120, 160, 1000, 4, True), (120, 160, 4000, 2, True), (120, 160, 1000, 4, False),
                                                      (122, 166, 1000, 2, False), (122, 166, 9999999, 1, False)])
@pytest.mark.parametrize("kind", ["identity", "motion", "rotation"])
def test_raw_lattice_equals_fp32_lattice(bt, kernel_cases, rows, cols, ns, stride, fast, kind):
    c = kernel_cases[(rows, cols)]
    lanes = 3
    n, lr, lc, st = device.error_lattice_size(rows, cols, ns)
    assert st == stride
    Rs, ts = warps(K_for(cols), lanes, kind)
    kf_lat = torch.zeros((lanes, 2 * n), device="cuda")
    bt.lattice_pack(c["W0"], c["I0"], ns, kf_lat)
    on = torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda")   # lane 1 masked off
    maps = (c["Wc"], c["W0"], c["Ic"], c["I0"])
    ref = torch.full((lanes, 2 * n + 8), 7.0, device="cuda")
    got = torch.full((lanes, 2 * n + 8), 7.0, device="cuda")
    bt.lattice_residuals_raw(*maps, Rs, ts, ns, ref, kf_lat, fast=fast, lane_on=on)
    bt.lattice_residuals_raw(*maps, Rs, ts, ns, got, kf_lat, fast=fast, depth_u16=c["depth"], rgb=c["rgb"], factor_depth=1.0, lane_on=on)
    assert same_bits(got, ref)
    # the masked lane and the tail are untouched; the fp32 variant of this entry is the existing entry's kernel
    assert bool((got[1] == 7.0).all()) and bool((got[:, 2 * n:] == 7.0).all())
    old = torch.full((lanes, 2 * n + 8), 7.0, device="cuda")
    bt.lattice_residuals(*maps, Rs, ts, ns, old, fast=fast, kf_lat=kf_lat)
    assert same_bits(old[0], ref[0]) and same_bits(old[2], ref[2])
    # the case has power: valid and invalid samples in both channels (the rotation loses a large part of the lattice)
    for l in (0, 2):
        nan = torch.isnan(ref[l, :2 * n]).float().view(2, n).mean(1)
        assert 0.02 < float(nan[0]) < 0.98 and 0.02 < float(nan[1]) < 0.98, (kind, l, nan)
        if kind == "rotation":
            assert float(nan[1]) > 0.25
    # unmasked, all three lanes
    bt.lattice_residuals_raw(*maps, Rs, ts, ns, got, kf_lat, fast=fast, depth_u16=c["depth"], rgb=c["rgb"], factor_depth=1.0)
    assert same_bits(got, old)


# ---- 3. the engine -----------------------------------------------------------------------------------------------------------------------------
def run_engine(ctx, depth, rgb, raw, prologue_lanes, unfed=None, **cfg_kw):
    """records, keyframe maps and exported keyframes of a run; raw: the RGBID_ENGINE_LATTICE_RAW setting (None: unset, the default)"""
    keys = {"RGBID_ENGINE_LATTICE_RAW": raw, "RGBID_ENGINE_UPDATE_PROLOGUE_LANES": prologue_lanes}
    old = {k: os.environ.get(k) for k in keys}
    T, B, rows, cols = depth.shape
    try:
        for k, v in keys.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        cfg = cfg_kw.pop("cfg", None)
        if cfg is None:
            cfg = E.default_config(rows=rows, cols=cols, lanes=B, record_capacity=T, keyframe_capacity=4, visratio_odo=0.985, visratio_integr=0.97, **cfg_kw)
        eng = E.Engine(ctx, cfg)
        for k in range(T):
            if unfed is not None:
                eng.set_active([0 if (k, l) == unfed else 1 for l in range(B)])
            eng.step(depth[k], rgb[k])
        rec = eng.records().copy()
        maps = [np.concatenate([m.reshape(-1).view(np.uint8) for m in eng.keyframe_maps(l)]) for l in range(B)]
        counts = [int(v) for v in eng.keyframe_counts()]
        kfs = []
        for l in range(B):
            for i in range(max(0, counts[l] - 4), counts[l]):
                a = eng.read_keyframe(l, i)
                kfs.append(b"".join(np.ascontiguousarray(a[k]).tobytes() for k in sorted(a) if isinstance(a[k], np.ndarray)) + repr((a["id"], a["end_id"], a["lane"], a["seq"])).encode())
        eng.close()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return rec, maps, counts, kfs


def assert_same_run(a, b):
    assert a[0].tobytes() == b[0].tobytes(), "pose records"
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1])), "keyframe maps"
    assert a[2] == b[2] and a[3] == b[3], "exported keyframes"


@pytest.fixture(scope="module")
def engine_frames():
    from tests.test_gpu_engine import make_lanes
    K = (131.25, 131.25, 79.5, 59.5)
    seqs, depth, rgb = make_lanes(3, 6, 120, 160, K, trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
    return K, depth, rgb


@pytest.mark.parametrize("use_graph", [0, 1])
def test_engine_raw_lattice_is_bit_identical(ctx, engine_frames, use_graph):
    """3 lanes, 120 x 160, the few-lane plan off (it keeps the fp32 maps and would hide the raw source at 3 lanes); lane 1 is not fed in step 2: its slice of the
    input buffer is stale then, and it does not iterate.  Eager (the caller's dense buffers) and graph mode (the pitched staging copies).  Six frames
    instead of four in eager mode: the sequences export keyframes by then (test_engine_records_do_not_depend_on_the_map_placement)"""
    K, depth, rgb = engine_frames
    T = 4 if use_graph else 6
    runs = [run_engine(ctx, depth[:T], rgb[:T], raw, "0", unfed=(2, 1), K=K, use_graph=use_graph) for raw in (None, "0", "1")]
    assert_same_run(runs[0], runs[1])
    assert_same_run(runs[2], runs[1])
    rec = runs[0][0]
    assert rec[2, 1]["status"] == 0 and np.count_nonzero(rec["status"] & E.ST_TRACKED) >= 3 * (T - 2)
    if not use_graph:
        assert sum(runs[0][2]) > 0    # keyframes were exported


@pytest.mark.parametrize("what", ["default environment (few-lane plan)", "exact class", "custom registration"])
def test_engine_raw_lattice_fallbacks_are_bit_identical(ctx, engine_frames, what):
    """configurations in which level 0 keeps the fp32 maps: the switch must change nothing"""
    K, depth, rgb = engine_frames
    kw, prologue = dict(K=K, use_graph=0), "0"
    if what.startswith("default"):
        prologue = None
    elif what == "exact class":
        kw["fast_numerics"] = 0
    else:
        import ctypes as C
        from rgbid import _lib
        from rgbid.device import IntrK, depth_dist
        cfg = E.default_config(rows=120, cols=160, lanes=3, K=K, use_graph=0, record_capacity=4, keyframe_capacity=4, custom_registration=1)
        for i, v in enumerate((0.02, -0.04, 0.0005, -0.0004, 0.01)):
            cfg.rgb_dist[i] = v
        cfg.depth_intr = IntrK(571.0 / 4, 572.5 / 4, (316.0 + 0.5) / 4 - 0.5, (241.5 + 0.5) / 4 - 0.5, -0.015, 0.03, 0.0003, 0.0002, -0.008)
        cfg.depth_dist = depth_dist(c1=1.01, c0=-0.002, q0=(0.001, -0.002, 0.001, 0.0, 0.0005, -0.0004, 0.0, 0.0, 0.0), q1=(0.005, 0.01, 0.0, 0.0, -0.002, 0.001, 0.0, 0.0, 0.0))
        _lib.check(_lib.lib().rgbid_engine_config_set_stereo(C.byref(cfg), (C.c_float * 9)(0.99995, -0.008, 0.006, 0.00803, 0.99995, -0.005, -0.00596, 0.00505, 0.99997),
                                                             (C.c_float * 3)(0.0251, -0.0012, 0.0031)))
        kw = dict(cfg=cfg)
    a = run_engine(ctx, depth[:4], rgb[:4], None, prologue, **dict(kw))
    b = run_engine(ctx, depth[:4], rgb[:4], "0", prologue, **dict(kw))
    assert_same_run(a, b)
    assert np.count_nonzero(a[0]["status"] & E.ST_TRACKED) >= 3 * 2
