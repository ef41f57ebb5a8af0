"""The frame-preparation stencils (csrc/kernels_prep.hip, csrc/kernels_bilateral.hip) against the oracle on the cases of tests/prep_cases.py: every shape
at which a kernel's wave, strip, tile or grid arithmetic changes, with clean, sparse (ONE NaN placed from the kernel's geometry), 10 % holes, all-NaN,
count-rule and sentinel contents -- through the single-image calls (rgbid.device.Context) and the batched calls (rgbid.batched.Batched).  The reference
is pinned on the same cases by tests/test_cpu_prep_cases.py.  Bars, the project's existing ones:
  converters, Sobel, keep-copy, vertex map 0 ULP; normals 2 ULP; pyramid 4 ULP; EXACT bilateral 8 ULP; FAST bilateral 2e-6 relative -- the NaN pattern
  identical everywhere.
Then: the pyramid's all-valid fast path and the shared-weight bilateral byte for byte against the kernels without them (one fresh child process), 1e30
around every source view and a marker around every destination view, each lane of a many-lane launch against itself alone, and the two-map launches of
the engine against their one-map calls.  Every test loops over many small maps inside one id."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as O
from rgbid import batched as BT
from rgbid._lib import RgbidError
from tests import prep_cases as P
from tests import util
from tests.util import assert_bits, ulp_diff

pytestmark = pytest.mark.gpu

POISON, MARKER = 1e30, 7.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bt(ctx):
    return BT.Batched(ctx)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the cases are read-only


def stack(maps):
    return torch.from_numpy(np.stack([np.ascontiguousarray(m) for m in maps])).cuda()


def marked(*shape):
    return torch.full(shape, MARKER, device="cuda")


def sigma_of(which):
    """the tracker's range sigmas: 2 * 0.0025 on inverse depth, 3 on intensity"""
    return 3.0 if which == "I" else 2 * 0.0025


def chunks(seq, n):
    return [seq[i:i + n] for i in range(0, len(seq), n)]


def fill32(cases):
    """32 lanes from the cases of one shape (cycled): the FAST bilateral walks 60 rows per wave from 32 lanes on"""
    return [cases[i % len(cases)] for i in range(32)]


# ---- references, computed once ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_pyr(which, name):
    c = _case("pyr", which, name)
    return O.pyr_down(c.map)


@functools.lru_cache(maxsize=None)
def ref_bil(kind, which, name, sigma):
    return O.bilateral(P.sanitised(_case(kind, which, name).map), sigma)


@functools.lru_cache(maxsize=None)
def ref_grad(kind, which, name):
    return O.gradient(_case(kind, which, name).map)


@functools.lru_cache(maxsize=None)
def _index(kind, which):
    return {c.name: c for c in P.float_cases(kind, which)}


def _case(kind, which, name):
    return _index(kind, which)[name]


def rel_fast(got, ref, what):
    """the FAST bilateral's bar: identical NaN pattern, 2e-6 relative -> worst relative deviation"""
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, int(np.count_nonzero(np.isnan(got) != np.isnan(ref))))
    m = ~np.isnan(ref)
    if not m.any():
        return 0.0
    d = np.abs(got[m].astype(np.float64) - ref[m])
    assert (d <= 2e-6 * np.abs(ref[m]) + 1e-30).all(), (what, float((d / np.abs(ref[m])).max()))
    return float((d / np.maximum(np.abs(ref[m]), 1e-30)).max())


def bits_ulp(got, ref, max_ulp, what):
    assert_bits(got, ref, max_ulp, what)
    return ulp_diff(got, ref)[0]


# ---- the launches whose fast paths have a slow twin: run here and, with the twins switched on, in a child process -----------------------------------
def fast_family_outputs(bt):
    """-> {key: ndarray}: the batched pyramid on every pyr case (all cases of a shape as the lanes of one launch) and the batched FAST bilateral on every
    bil_fast case (three lanes a launch: 30 rows per wave) and bil_fast32 case (32 lanes: 60 rows per wave)"""
    out = {}
    for which in ("W", "I"):
        for (rows, cols), cases in P.by_shape(P.float_cases("pyr", which)).items():
            src = stack([c.map for c in cases])
            dst = marked(len(cases), rows // 2, cols // 2)
            bt.pyr_down(src, dst)
            out[f"pyr/{which}/{rows}x{cols}"] = dst.cpu().numpy()
        for kind in ("bil_fast", "bil_fast32"):
            for (rows, cols), cases in P.by_shape(P.float_cases(kind, which)).items():
                groups = chunks(cases, 3) if kind == "bil_fast" else [fill32(cases)]
                for i, g in enumerate(groups):
                    src = stack([c.map for c in g])
                    dst = marked(*src.shape)
                    bt.bilateral(src, dst, sigma_of(which), fast=True)
                    out[f"{kind}/{which}/{rows}x{cols}/{i}"] = dst.cpu().numpy()
    return out


_WORKER = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/rgbid-slam_amd")
from rgbid import device, batched
from tests import test_gpu_prep_paths as T
ctx = device.Context(0)
np.savez(sys.argv[2], **T.fast_family_outputs(batched.Batched(ctx)))
ctx.close()
"""


@pytest.fixture(scope="module")
def fast_outputs(bt):
    return fast_family_outputs(bt)


@pytest.fixture(scope="module")
def slow_twin_outputs(tmp_path_factory):
    """the same launches with RGBID_PYRDOWN_NO_FASTPATH and RGBID_BILATERAL_TWO_SIDED set: one fresh process, under a time limit"""
    path = str(tmp_path_factory.mktemp("prep_paths") / "twins.npz")
    env = dict(os.environ, RGBID_BILATERAL_TWO_SIDED="1", RGBID_PYRDOWN_NO_FASTPATH="1")
    subprocess.run([sys.executable, "-c", _WORKER, ROOT, path], check=True, env=env, timeout=300)
    return np.load(path)


def test_pyramid_fast_path_changes_no_byte(fast_outputs, slow_twin_outputs):
    """k_pyr_down_dpp skips tap count and mask sum where five wave-uniform `full[]` flags say so: on clean maps it runs everywhere but at the border, on sparse
    maps it switches off for the waves and rows that see the one NaN -- and the result is the slow path's, byte for byte, on every case"""
    n = 0
    for k, got in fast_outputs.items():
        if k.startswith("pyr/"):
            ref = slow_twin_outputs[k]
            assert got.tobytes() == ref.tobytes(), (k, int(np.count_nonzero(got.view(np.uint32) != ref.view(np.uint32))))
            n += got.shape[0]
    assert n > 1500


def test_shared_bilateral_equals_the_two_sided_kernel(fast_outputs, slow_twin_outputs):
    """k_bilateral_shared (30 and 60 rows per wave) against k_bilateral<2> byte for byte on every FAST case, the sentinel's neighbours included"""
    n = 0
    for k, got in fast_outputs.items():
        if k.startswith("bil_fast"):
            ref = slow_twin_outputs[k]
            assert got.tobytes() == ref.tobytes(), (k, int(np.count_nonzero(got.view(np.uint32) != ref.view(np.uint32))))
            n += got.shape[0]
    assert n > 1500


# ---- every case against the oracle -------------------------------------------------------------------------------------------------------------
def test_pyramid_cases(ctx, fast_outputs):
    worst, n = 0, 0
    for which in ("W", "I"):
        for (rows, cols), cases in P.by_shape(P.float_cases("pyr", which)).items():
            batched = fast_outputs[f"pyr/{which}/{rows}x{cols}"]
            for l, c in enumerate(cases):
                ref = ref_pyr(which, c.name)
                dst = marked(rows // 2, cols // 2)
                ctx.pyrDown(dev(c.map), dst)
                worst = max(worst, bits_ulp(dst.cpu().numpy(), ref, 4, c.name), bits_ulp(batched[l], ref, 4, c.name + " (batched)"))
                if c.content == "count":
                    for y, x, k in c.meta:
                        assert np.isnan(batched[l][y, x]) == (k == 12), (c.name, y, x, k)
                n += 1
    print(f"pyrDown: {n} cases, single and batched, worst {worst} ULP")
    assert n > 1500


def test_fast_bilateral_cases(ctx, fast_outputs):
    worst, n = 0.0, 0
    for which in ("W", "I"):
        sigma = sigma_of(which)
        for kind in ("bil_fast", "bil_fast32"):
            for (rows, cols), cases in P.by_shape(P.float_cases(kind, which)).items():
                groups = chunks(cases, 3) if kind == "bil_fast" else [fill32(cases)]
                for i, g in enumerate(groups):
                    got = fast_outputs[f"{kind}/{which}/{rows}x{cols}/{i}"]
                    for l, c in enumerate(g):
                        worst = max(worst, rel_fast(got[l], ref_bil(kind, which, c.name, sigma), c.name + " (batched)")); n += 1
                if kind == "bil_fast32":
                    continue
                ctx.set_numerics(True)
                try:
                    for c in cases:
                        dst = marked(rows, cols)
                        ctx.bilateralFilter(dev(c.map), dst, sigma)
                        worst = max(worst, rel_fast(dst.cpu().numpy(), ref_bil(kind, which, c.name, sigma), c.name))
                finally:
                    ctx.set_numerics(False)
    print(f"FAST bilateral: {n} lanes, worst relative {worst:.2e}")
    assert n > 1500


def test_exact_bilateral_cases(ctx, bt):
    worst = {}
    n = 0
    for which, sigma in P.EXACT_SIGMAS:
        for (rows, cols), cases in P.by_shape(P.float_cases("bil_exact", which)).items():
            src = stack([c.map for c in cases])
            dst = marked(*src.shape)
            bt.bilateral(src, dst, sigma, fast=False)
            got = dst.cpu().numpy()
            for l, c in enumerate(cases):
                ref = ref_bil("bil_exact", which, c.name, sigma)
                one = marked(rows, cols)
                ctx.bilateralFilter(dev(c.map), one, sigma)
                u = max(bits_ulp(got[l], ref, 8, c.name + " (batched)"), bits_ulp(one.cpu().numpy(), ref, 8, c.name))
                worst[sigma] = max(worst.get(sigma, 0), u); n += 1
    print(f"EXACT bilateral: {n} cases, worst ULP per sigma {worst}")
    assert n > 500


def _check_grad(gx, gy, ref, what):
    assert_bits(gx, ref[0], 0, what + " gx"); assert_bits(gy, ref[1], 0, what + " gy")


def test_sobel_and_keep_cases(ctx, bt):
    n = 0
    for kind in ("sobel16", "sobelfb"):
        for which in (("W", "I") if kind == "sobel16" else ("W",)):
            for (rows, cols), cases in P.by_shape(P.float_cases(kind, which)).items():
                src = stack([c.map for c in cases])
                gx, gy, keep = marked(*src.shape), marked(*src.shape), marked(*src.shape)
                bt.gradient(src, gx, gy)
                hx, hy = gx.cpu().numpy(), gy.cpu().numpy()
                if kind == "sobel16":
                    kx, ky = marked(*src.shape), marked(*src.shape)
                    bt.gradient_keep(src, kx, ky, keep)
                    assert kx.cpu().numpy().tobytes() == hx.tobytes() and ky.cpu().numpy().tobytes() == hy.tobytes(), (kind, rows, cols)
                    assert keep.cpu().numpy().tobytes() == src.cpu().numpy().tobytes(), (kind, rows, cols)      # NaN payloads included
                else:
                    with pytest.raises(RgbidError, match="rgbid error -1"):      # off the 16-byte path: refused, never another kernel
                        bt.gradient_keep(src, gx.clone(), gy.clone(), keep)
                for l, c in enumerate(cases):
                    ref = ref_grad(kind, which, c.name)
                    _check_grad(hx[l], hy[l], ref, c.name + " (batched)")
                    ox, oy = marked(rows, cols), marked(rows, cols)
                    ctx.computeGradient(dev(c.map), ox, oy)
                    _check_grad(ox.cpu().numpy(), oy.cpu().numpy(), ref, c.name)
                    n += 1
    print(f"Sobel: {n} cases, single and batched, 0 ULP")
    assert n > 900


def test_sobel_of_a_view_off_the_16_byte_grid(ctx, bt):
    """a width that is a multiple of 4 in a view that starts one float into its allocation: k_gradient instead of k_gradient4, the same bits"""
    rows, cols = P.MISALIGNED_SHAPE
    maps = [P.base_map("sobel16", rows, cols, "W", 11 + i) for i in range(3)]
    maps[1][5, 7] = np.nan
    aligned = stack(maps)
    big = torch.full((3, rows, cols + 8), POISON, device="cuda")
    view = big[:, :, 1:1 + cols]
    view.copy_(aligned)
    assert view.data_ptr() % 16 == 4 and aligned.data_ptr() % 16 == 0
    outs = [[marked(3, rows, cols) for _ in range(2)] for _ in range(2)]
    bt.gradient(aligned, *outs[0])
    bt.gradient(view, *outs[1])
    for a, b in zip(outs[0], outs[1]):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    for l in range(3):
        _check_grad(outs[1][0][l].cpu().numpy(), outs[1][1][l].cpu().numpy(), O.gradient(maps[l]), f"view lane {l}")
    with pytest.raises(RgbidError, match="rgbid error -1"):
        bt.gradient_keep(view, marked(3, rows, cols), marked(3, rows, cols), marked(3, rows, cols))
    one_x, one_y = marked(rows, cols), marked(rows, cols)
    ctx.computeGradient(view[1], one_x, one_y)
    _check_grad(one_x.cpu().numpy(), one_y.cpu().numpy(), O.gradient(maps[1]), "view, single image")


def _check_kf(gv, gn, w, K, what):
    """-> worst normal ULP.  Vertex map 0 ULP, normals 2 ULP; planes 1 / 2 where the reference defines them (NaN elsewhere when `nan_fill`)"""
    rows = w.shape[0]
    ov = O.vmap(w, K)
    gx, gy = O.gradient(w)
    on = O.nmap_gradients(w, gx, gy, K)
    valid, nvalid = ~np.isnan(ov[:rows]), ~np.isnan(on[:rows])
    assert_bits(gv[:rows], ov[:rows], 0, what + " vmap x")
    worst = bits_ulp(gn[:rows], on[:rows], 2, what + " nmap x")
    for p in (1, 2):
        sl = slice(p * rows, (p + 1) * rows)
        assert_bits(gv[sl][valid], ov[sl][valid], 0, f"{what} vmap plane {p}")
        worst = max(worst, bits_ulp(gn[sl][nvalid], on[sl][nvalid], 2, f"{what} nmap plane {p}"))
    return worst, valid, nvalid


def test_keyframe_map_cases(ctx, bt):
    worst, n = 0, 0
    for (rows, cols), cases in P.by_shape(P.kf_cases()).items():
        K = cases[0].meta
        src = stack([c.map for c in cases])
        vm, nm = marked(len(cases), 3 * rows, cols), marked(len(cases), 3 * rows, cols)
        bt.kf_maps(K, src, vm, nm)
        gv, gn = vm.cpu().numpy(), nm.cpu().numpy()
        for l, c in enumerate(cases):
            u, valid, nvalid = _check_kf(gv[l], gn[l], c.map, K, c.name + " (batched)")
            for p in (1, 2):      # the fused kernel writes NaN where the reference leaves the plane untouched
                assert np.isnan(gv[l][p * rows:(p + 1) * rows][~valid]).all() and np.isnan(gn[l][p * rows:(p + 1) * rows][~nvalid]).all(), c.name
            ov, on_ = marked(3 * rows, cols), marked(3 * rows, cols)
            ctx.createVMap(K, dev(c.map), ov)
            gx, gy = O.gradient(c.map)
            ctx.createNMapGradients(K, dev(c.map), dev(gx), dev(gy), on_)
            u1, _, _ = _check_kf(ov.cpu().numpy(), on_.cpu().numpy(), c.map, K, c.name)
            worst = max(worst, u, u1); n += 1
    print(f"keyframe maps: {n} cases, vertex map 0 ULP, normals worst {worst} ULP")
    assert n == 4 * len(P.SHAPES["sobel16"])
    for rows, cols in ((4, 3), (65, 66)):      # off the 16-byte path: the fused kernel refuses, the engine then runs the three kernels
        with pytest.raises(RgbidError, match="rgbid error -1"):
            bt.kf_maps(P.K_for(rows, cols), marked(1, rows, cols), marked(1, 3 * rows, cols), marked(1, 3 * rows, cols))


def test_prep_frame_cases(ctx, bt):
    for c in P.prep_cases():
        d16 = dev(c.depth.view(np.int16)); rgb = dev(c.rgb)
        for factor in (1.0, 0.96):
            refs = [O.depth2invdepth(c.depth, factor), O.intensity(c.rgb)] + list(O.decompose_rgb(c.rgb))
            outs = [marked(1, c.rows, c.cols) for _ in range(5)]
            bt.prep_frame(d16[None], rgb[None], *outs, factor)
            for got, ref, what in zip(outs, refs, ("iD", "luma", "r", "g", "b")):
                assert_bits(got[0].cpu().numpy(), ref, 0, f"{c.name} {what} (batched, factor {factor})")
            one = [marked(c.rows, c.cols) for _ in range(5)]
            ctx.convertDepth2InvDepth(d16, one[0], factor)
            ctx.computeIntensity(rgb, one[1])
            ctx.decomposeRGBInChannels(rgb, *one[2:])
            for got, ref, what in zip(one, refs, ("iD", "luma", "r", "g", "b")):
                assert_bits(got.cpu().numpy(), ref, 0, f"{c.name} {what} (factor {factor})")
    # several lanes: the grid-stride loop per lane (blockIdx.y)
    cs = [c for c in P.prep_cases() if (c.rows, c.cols) == (513, 4)] * 3
    outs = [marked(3, 513, 4) for _ in range(5)]
    bt.prep_frame(stack([c.depth.view(np.int16) for c in cs]), stack([c.rgb for c in cs]), *outs, 1.0)
    for l in range(3):
        assert_bits(outs[0][l].cpu().numpy(), O.depth2invdepth(cs[l].depth, 1.0), 0, "iD lanes")
        assert_bits(outs[1][l].cpu().numpy(), O.intensity(cs[l].rgb), 0, "luma lanes")


# ---- poison around the sources, markers around the destinations --------------------------------------------------------------------------------
def poisoned(t, fill=POISON, top=1, bottom=2, right=4):
    """t [lanes, rows, cols(, 3)] as a view into a taller and wider allocation filled with `fill`: rows above and below every lane, columns directly behind
    the last column of every row.  right = 4 floats keeps a 16-byte geometry on the 16-byte path.  -> (view, allocation)"""
    L, rows, cols = t.shape[:3]
    big = torch.full((L, rows + top + bottom, cols + right) + tuple(t.shape[3:]), fill, dtype=t.dtype, device="cuda")
    v = big[:, top:top + rows, :cols]
    v.copy_(t)
    return v, big


def intact(view_big, rows, cols, top=1, fill=MARKER):
    """every element of the allocation outside the view still holds the marker"""
    v, big = view_big
    mask = torch.ones(big.shape, dtype=torch.bool, device="cuda")
    mask[:, top:top + rows, :cols] = False
    return bool((big[mask] == fill).all())


def _picked(cases):
    """clean, the first and the last sparse, holes"""
    sp = [c for c in cases if c.content == "sparse"]
    return [c for c in cases if c.content in ("clean", "holes", "count", "special")] + sp[:1] + sp[-1:]


def _run_poisoned(call, srcs, dst_shapes):
    """call(sources..., destinations...) plain and poisoned -> the same bits in the destinations, the markers around them intact"""
    plain = [marked(*s) for s in dst_shapes]
    call(*srcs, *plain)
    psrc = [poisoned(s)[0] for s in srcs]
    pdst = [poisoned(marked(*s), fill=MARKER) for s in dst_shapes]
    call(*psrc, *[v for v, _ in pdst])
    for a, (v, big), s in zip(plain, pdst, dst_shapes):
        assert a.cpu().numpy().tobytes() == v.contiguous().cpu().numpy().tobytes(), "padding changed the result"
        assert intact((v, big), s[1], s[2]), "a marker outside the destination view was overwritten"
    return plain


def test_poison_around_sources_and_markers_around_destinations(bt):
    """sources are views into wider and taller allocations whose padding holds 1e30 (directly behind the last column of every row: what the pyramid's
    8-byte pair load reads at an odd width), destinations views into marker-filled allocations: the bits of the unpadded run, every marker intact"""
    n = 0
    for which in ("W", "I"):
        sigma = sigma_of(which)
        for (rows, cols), cases in P.by_shape(P.float_cases("pyr", which)).items():
            src = stack([c.map for c in _picked(cases)])
            _run_poisoned(bt.pyr_down, [src], [(src.shape[0], rows // 2, cols // 2)]); n += 1
        for (rows, cols), cases in P.by_shape(P.float_cases("bil_fast", which)).items():
            src = stack([c.map for c in _picked(cases)][:3])
            _run_poisoned(lambda s, d: bt.bilateral(s, d, sigma, fast=True), [src], [tuple(src.shape)]); n += 1
        for (rows, cols), cases in P.by_shape(P.float_cases("bil_fast32", which)).items():
            src = stack([c.map for c in fill32(_picked(cases))])
            _run_poisoned(lambda s, d: bt.bilateral(s, d, sigma, fast=True), [src], [tuple(src.shape)]); n += 1
        for (rows, cols), cases in P.by_shape(P.float_cases("bil_exact", which)).items():
            src = stack([c.map for c in _picked(cases)])
            for sg in ((sigma, 0.02) if which == "W" else (sigma,)):
                _run_poisoned(lambda s, d: bt.bilateral(s, d, sg, fast=False), [src], [tuple(src.shape)]); n += 1
        for kind in ("sobel16", "sobelfb"):
            if kind == "sobelfb" and which == "I":
                continue
            for (rows, cols), cases in P.by_shape(P.float_cases(kind, which)).items():
                src = stack([c.map for c in _picked(cases)])
                _run_poisoned(bt.gradient, [src], [tuple(src.shape)] * 2); n += 1
                if kind == "sobel16":
                    _run_poisoned(bt.gradient_keep, [src], [tuple(src.shape)] * 3); n += 1
    for (rows, cols), cases in P.by_shape(P.kf_cases()).items():
        src = stack([c.map for c in cases])
        K = cases[0].meta
        # the three planes of a vertex / normal map are one view of 3 * rows rows
        _run_poisoned(lambda s, v, m: bt.kf_maps(K, s, v, m), [src], [(src.shape[0], 3 * rows, cols)] * 2); n += 1
    for c in P.prep_cases():
        d16 = dev(c.depth.view(np.int16))[None]; rgb = dev(c.rgb)[None]
        plain = [marked(1, c.rows, c.cols) for _ in range(5)]
        bt.prep_frame(d16, rgb, *plain, 0.96)
        pd, _ = poisoned(d16, fill=30000); pc, _ = poisoned(rgb, fill=201)
        pdst = [poisoned(marked(1, c.rows, c.cols), fill=MARKER) for _ in range(5)]
        bt.prep_frame(pd, pc, *[v for v, _ in pdst], 0.96)
        for a, (v, big) in zip(plain, pdst):
            assert a.cpu().numpy().tobytes() == v.contiguous().cpu().numpy().tobytes() and intact((v, big), c.rows, c.cols), c.name
        n += 1
    assert n > 300


# ---- lanes --------------------------------------------------------------------------------------------------------------------------------------
def test_every_lane_equals_itself_alone(bt):
    """7, 8, 9 and 17 lanes of different 16 x 124 maps through the pyramid are grids of 7, 8, 9 and 17 workgroups: xcd_slab_index without a renumbered part, without
    a tail, and with tails of 1.  31 and 32 lanes of different 61 x 61 and 241 x 61 maps through the FAST bilateral: 30 and 60 rows per wave.  Each lane equals
    itself run alone, bit for bit -- so the first 31 lanes of the two bilateral runs equal each other: the rows-per-wave switch changes nothing."""
    maps = []
    for l in range(17):
        a = P.base_map("pyr", 16, 124, "WI"[l % 2], 20 + l)
        if l % 3 == 1:
            a[(5 * l) % 16, (37 * l) % 124] = np.nan      # sparse: the fast path is off in some lanes' waves only
        if l % 3 == 2:
            a[util.rng(77 + l).random(a.shape) < 0.1] = np.nan
        maps.append(a)
    alone = []
    for a in maps:
        d = marked(1, 8, 62)
        bt.pyr_down(stack([a]), d)
        alone.append(d.cpu().numpy()[0])
    for lanes in (7, 8, 9, 17):
        d = marked(lanes, 8, 62)
        bt.pyr_down(stack(maps[:lanes]), d)
        got = d.cpu().numpy()
        for l in range(lanes):
            assert got[l].tobytes() == alone[l].tobytes(), ("pyrDown", lanes, l)
            assert_bits(got[l], O.pyr_down(maps[l]), 4, f"pyrDown lane {l} of {lanes}")
    for rows, cols in ((61, 61), (241, 61)):
        maps = []
        for l in range(32):
            a = P.base_map("bil_fast32", rows, cols, "I", 40 + l)
            if l % 2:
                a[util.rng(88 + l).random(a.shape) < 0.05] = np.nan
            if l % 5 == 0:
                a[(7 * l + 58) % rows, (11 * l) % cols] = 1e19
            maps.append(a)
        alone = []
        for a in maps:
            d = marked(1, rows, cols)
            bt.bilateral(stack([a]), d, 3.0, fast=True)
            alone.append(d.cpu().numpy()[0])
        runs = {}
        for lanes in (31, 32):
            d = marked(lanes, rows, cols)
            bt.bilateral(stack(maps[:lanes]), d, 3.0, fast=True)
            runs[lanes] = d.cpu().numpy()
            for l in range(lanes):
                assert runs[lanes][l].tobytes() == alone[l].tobytes(), ("bilateral", rows, cols, lanes, l)
        assert runs[31].tobytes() == runs[32][:31].tobytes()
        for l in (0, 15, 31):
            rel_fast(runs[32][l], O.bilateral(P.sanitised(maps[l]), 3.0), f"bilateral lane {l}")


# ---- the engine's two-map launches ------------------------------------------------------------------------------------------------------------
def _pair_maps(rows, cols, lanes, seed):
    W = [util.rand_invdepth(util.rng(seed + l), rows, cols, nan_frac=0.05 if l % 2 == 0 else 0.0) for l in range(lanes)]
    I = [util.rand_intensity(util.rng(seed + 50 + l), rows, cols, nan_frac=0.0 if l % 2 == 0 else 0.02) for l in range(lanes)]
    if lanes > 1:
        W[1][rows // 2, cols // 2] = np.nan         # a single hole: the pyramid's fast path switches inside the second map's half of the grid too
    return W, I


PAIR_GEOMS = [(16, 124, 1), (16, 124, 3), (16, 124, 9), (61, 83, 2), (480, 120, 1), (480, 121, 1), (64, 64, 2), (129, 64, 2)]


def _same(a, b, what):
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), what


def test_two_map_launches_equal_two_one_map_calls(bt):
    """launch_pyr_down2 / launch_bilateral2 / launch_gradient2 / launch_gradient_keep2 -- all the engine and kfalign.hip ever call -- through their own entry
    points: the second map's indexing (`V -= wgs_per_map`, `tid_.by >= ny`, blockIdx.z) gives the bits of two one-map calls, and both halves meet the oracle"""
    for rows, cols, lanes in PAIR_GEOMS:
        W, I = _pair_maps(rows, cols, lanes, 3000 + rows + cols)
        sW, sI = stack(W), stack(I)
        what = f"{rows}x{cols}x{lanes}"
        # pyramid
        half = (lanes, rows // 2, cols // 2)
        p0, p1, q0, q1 = [marked(*half) for _ in range(4)]
        bt.pyr_down_pair(sW, p0, sI, p1)
        bt.pyr_down(sW, q0); bt.pyr_down(sI, q1)
        _same(p0, q0, "pyr pair, first map " + what); _same(p1, q1, "pyr pair, second map " + what)
        for l in range(lanes):
            assert_bits(p0[l].cpu().numpy(), O.pyr_down(W[l]), 4, "pyr pair W"); assert_bits(p1[l].cpu().numpy(), O.pyr_down(I[l]), 4, "pyr pair I")
        # bilateral, both classes, each map its own sigma
        for fast in (True, False):
            b0, b1, c0, c1 = [marked(*sW.shape) for _ in range(4)]
            bt.bilateral_pair(sW, b0, 2 * 0.0025, sI, b1, 3.0, fast=fast)
            bt.bilateral(sW, c0, 2 * 0.0025, fast=fast); bt.bilateral(sI, c1, 3.0, fast=fast)
            _same(b0, c0, f"bilateral pair fast={fast}, first map " + what); _same(b1, c1, f"bilateral pair fast={fast}, second map " + what)
            for l in range(lanes):
                for got, src, sg in ((b0, W[l], 2 * 0.0025), (b1, I[l], 3.0)):
                    ref = O.bilateral(src, sg)
                    if fast:
                        rel_fast(got[l].cpu().numpy(), ref, "bilateral pair " + what)
                    else:
                        assert_bits(got[l].cpu().numpy(), ref, 8, "bilateral pair " + what)
        # Sobel, and Sobel + keep
        g = [marked(*sW.shape) for _ in range(8)]
        bt.gradient_pair(sW, g[0], g[1], sI, g[2], g[3])
        bt.gradient(sW, g[4], g[5]); bt.gradient(sI, g[6], g[7])
        for i in range(4):
            _same(g[i], g[4 + i], f"gradient pair output {i} " + what)
        for l in range(lanes):
            _check_grad(g[0][l].cpu().numpy(), g[1][l].cpu().numpy(), O.gradient(W[l]), "gradient pair W")
            _check_grad(g[2][l].cpu().numpy(), g[3][l].cpu().numpy(), O.gradient(I[l]), "gradient pair I")
        k = [marked(*sW.shape) for _ in range(6)]
        if cols % 4 == 0:
            bt.gradient_keep_pair(sW, k[0], k[1], k[2], sI, k[3], k[4], k[5])
            for i, j in ((0, 4), (1, 5), (3, 6), (4, 7)):
                _same(k[i], g[j], f"gradient keep pair output {i} " + what)
            _same(k[2], sW, "keep W " + what); _same(k[5], sI, "keep I " + what)
        else:
            with pytest.raises(RgbidError, match="rgbid error -1"):
                bt.gradient_keep_pair(sW, k[0], k[1], k[2], sI, k[3], k[4], k[5])


def test_two_map_launches_fall_back_on_unlike_pairs(bt):
    """two maps of unlike geometry, or two sigmas that need different EXACT kernels: the launcher takes the one-map path for each, the same bits"""
    W, _ = _pair_maps(16, 124, 2, 4100)
    _, I = _pair_maps(18, 124, 2, 4200)
    sW, sI = stack(W), stack(I)
    p0, q0 = marked(2, 8, 62), marked(2, 8, 62)
    p1, q1 = marked(2, 9, 62), marked(2, 9, 62)
    bt.pyr_down_pair(sW, p0, sI, p1)
    bt.pyr_down(sW, q0); bt.pyr_down(sI, q1)
    _same(p0, q0, "pyr"); _same(p1, q1, "pyr")
    assert_bits(p1[1].cpu().numpy(), O.pyr_down(I[1]), 4, "pyr, unlike pair")
    for fast in (True, False):
        b0, c0, b1, c1 = marked(*sW.shape), marked(*sW.shape), marked(*sI.shape), marked(*sI.shape)
        bt.bilateral_pair(sW, b0, 2 * 0.0025, sI, b1, 3.0, fast=fast)
        bt.bilateral(sW, c0, 2 * 0.0025, fast=fast); bt.bilateral(sI, c1, 3.0, fast=fast)
        _same(b0, c0, "bilateral"); _same(b1, c1, "bilateral")
    g = [marked(*(sW.shape if i % 4 < 2 else sI.shape)) for i in range(8)]
    bt.gradient_pair(sW, g[0], g[1], sI, g[2], g[3])
    bt.gradient(sW, g[4], g[5]); bt.gradient(sI, g[6], g[7])
    for i in range(4):
        _same(g[i], g[4 + i], "gradient")
    k = [marked(*(sW.shape if i < 3 else sI.shape)) for i in range(6)]
    bt.gradient_keep_pair(sW, k[0], k[1], k[2], sI, k[3], k[4], k[5])
    for i, j in ((0, 4), (1, 5), (3, 6), (4, 7)):
        _same(k[i], g[j], "gradient keep")
    _same(k[2], sW, "keep"); _same(k[5], sI, "keep")
    # one verified range sigma (k_bilateral<1>) beside one that is not (k_bilateral<0>): two launches; two unverified ones: one k_bilateral<0> launch
    W2, _ = _pair_maps(33, 65, 2, 4300)
    s0, s1 = stack(W), stack(W2)
    for sg0, sg1, a, b in ((2 * 0.0025, 0.02, sW, sW.flip(0).contiguous()), (0.02, 0.03, s1, s1.flip(0).contiguous())):
        b0, b1, c0, c1 = [marked(*a.shape) for _ in range(4)]
        bt.bilateral_pair(a, b0, sg0, b, b1, sg1, fast=False)
        bt.bilateral(a, c0, sg0, fast=False); bt.bilateral(b, c1, sg1, fast=False)
        _same(b0, c0, "EXACT bilateral, mixed sigmas"); _same(b1, c1, "EXACT bilateral, mixed sigmas")
        assert_bits(b1[0].cpu().numpy(), O.bilateral(b[0].cpu().numpy(), sg1), 8, "EXACT bilateral, second sigma")


def test_refusals_at_the_smallest_shapes(ctx, bt):
    """what an entry point cannot take it refuses with RGBID_E_INVALID (-1) -- it never runs another kernel quietly"""
    inv = dict(match="rgbid error -1")
    with pytest.raises(RgbidError, **inv):      # a one-column source has no destination column
        bt.pyr_down(marked(1, 2, 1), torch.empty((1, 1, 0), device="cuda"))
    with pytest.raises(RgbidError, **inv):
        bt.pyr_down(marked(1, 4, 4), marked(1, 2, 1))
    with pytest.raises(RgbidError, **inv):
        bt.pyr_down_pair(marked(1, 4, 4), marked(1, 2, 2), marked(1, 4, 4), marked(1, 2, 1))
    with pytest.raises(RgbidError, **inv):
        bt.bilateral_pair(marked(1, 4, 4), marked(1, 4, 4), 3.0, marked(1, 4, 4), marked(1, 4, 4), 0.0, fast=True)
    with pytest.raises(RgbidError, **inv):
        bt.gradient_pair(marked(1, 4, 4), marked(1, 4, 4), marked(1, 4, 4), marked(1, 4, 4), marked(1, 4, 4), marked(1, 3, 4))
    a = marked(1, 1, 4)
    with pytest.raises(RgbidError, **inv):      # keep must not be the source
        bt.gradient_keep_pair(a, marked(1, 1, 4), marked(1, 1, 4), a, marked(1, 1, 4), marked(1, 1, 4), marked(1, 1, 4), marked(1, 1, 4))
    # the smallest shapes every stencil does take: 1 x 1 bilateral and Sobel, 2 x 2 pyramid (one output, a corner window: invalid)
    one = dev(np.array([[[0.5]]], np.float32))
    d = marked(1, 1, 1)
    bt.bilateral(one, d, 3.0, fast=True); assert float(d[0, 0, 0]) == 0.5
    bt.bilateral(one, d, 3.0, fast=False); assert float(d[0, 0, 0]) == 0.5
    gx, gy = marked(1, 1, 1), marked(1, 1, 1)
    bt.gradient(one, gx, gy); assert float(gx[0, 0, 0]) == 0.0 and float(gy[0, 0, 0]) == 0.0
    p = marked(1, 1, 1)
    bt.pyr_down(marked(1, 2, 2), p); assert bool(torch.isnan(p).all())
