"""The robust-scale kernels (csrc/sigma_device.h, csrc/kernels_sigma.hip) at the sample counts where their paths change, on the residual sets of
tests/sigma_cases.py (tests/test_cpu_sigma_cases.py pins the reference on them to a tenth of the bars used here):

  k_sigma<REG>              ctx.computeSigmaAndNuStudent (mode 0), ctx.computeNuStudent (mode 1), ctx.computeSigmaPdf (mode 2, four M-estimators)
  k_sigma_pair_arrays<REG>  bt.sigma_pair: both channels of every lane in one launch, what the engine runs
  k_sigma_pair<REG>         bt.sigma_pair_maps: the lattice sampled from four maps through LatticeGetter's cursor
  k_chi_square              ctx.computeChiSquare

Bars (the ones tests/test_gpu_kernels.py and tests/test_gpu_batched.py use): bias and sigma within 2e-5 sigma of the oracle and nu equal on DECIDED cases
(sigma_cases.decided_student / decided_pdf); on undecided ones sigma within 2e-2 relative and nu a value of the bisection grid (tests/test_gpu_engine.py's
bound); chi-square: the count exact, chi within 2e-5 relative, the tail value within 1e-5.  Where the oracle is not finite the device gives NaN for NaN
and an inf of the same sign for inf.

Besides the values: nothing behind sample n is read (finite poison, 1e30, behind every array, between lanes and in the other channel's place: the
results do not change by a bit -- NaN padding would be sanitised away and prove nothing), lanes do not see each other, and the map-sampling kernel gives
the bits of the array kernel on the oracle's lattice of the same maps.

Run with -s to see the worst deviation per entry point and path and the number of undecided cases.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from rgbid import batched as BT
from rgbid import device
from tests import sigma_cases as SC

pytestmark = pytest.mark.gpu

BAR, WEAK_BAR = 2e-5, 2e-2
CHI_BAR, TAIL_BAR = 2e-5, 1e-5
POISON = np.float32(1e30)
HEAD, TAIL = 5, SC.REG_MAX + 4 * SC.SIG_T      # poison in front (the array then starts 4-byte aligned only) and behind: more than any slot of the register path could reach
ODD_COUNTS = tuple(n for n in SC.COUNTS if n % 2 == 1 and n > 3)
PAIR_KEYS = (("bias_depthinv", "sigma_depthinv", "nu_depthinv"), ("bias_int", "sigma_int", "nu_int"))

_worst = {}        # (entry point, path) -> (deviation of bias / sigma relative to sigma, case)
_undecided = {}    # entry point -> [undecided, total]


@pytest.fixture(scope="module")
def bt(ctx):
    return BT.Batched(ctx)


def dev(a):
    t = torch.from_numpy(np.array(a, copy=True)).cuda()      # a copy: the shared residual sets are read-only
    torch.cuda.synchronize()
    return t


def poisoned(e):
    """the same samples inside a larger allocation full of 1e30 -> a view of exactly e.size floats"""
    buf = np.full(HEAD + e.size + TAIL, POISON, np.float32)
    buf[HEAD:HEAD + e.size] = e
    return dev(buf)[HEAD:HEAD + e.size]


@functools.lru_cache(maxsize=None)
def decided_student(n, s, c, mest):
    with np.errstate(all="ignore"):
        return SC.decided_student(O.sigma_nu_student, SC.residuals(n, s, c), SC.start_sigma(s), mest)[0]


@functools.lru_cache(maxsize=None)
def oracle_student(n, s, c, mest):
    with np.errstate(all="ignore"):
        return O.sigma_nu_student(SC.residuals(n, s, c), 0.0, SC.start_sigma(s), 5.0, mest)


def hold(fails, entry, n, what, got, ref, decided):
    """(bias, sigma[, nu]) of the device against the oracle's under the module's bars; counts and records.  A miss goes into `fails` (the caller asserts
    that list empty at its end, so one run shows every case that misses)"""
    u = _undecided.setdefault(entry, [0, 0])
    u[1] += 1
    u[0] += 0 if decided else 1
    (gb, gs), (ob, os_) = got[:2], ref[:2]
    bad = []
    for g, o, name in ((gb, ob, "bias"), (gs, os_, "sigma")):
        if not np.isfinite(o) and not SC.same_nonfinite(g, o):
            bad.append(f"{name} {g} where the oracle has {o}")
    if np.isfinite(os_):
        if not np.isfinite(gs):
            bad.append(f"sigma {gs} where the oracle has {os_}")
        elif decided:
            ds = abs(gs - os_)
            db = abs(gb - ob) if np.isfinite(ob) else 0.0
            if np.isfinite(ob) and not np.isfinite(gb):
                bad.append(f"bias {gb} where the oracle has {ob}")
            elif not (ds <= BAR * os_ and db <= BAR * os_):
                bad.append(f"bias off by {db / os_ if os_ else db:.2e}, sigma by {ds / os_ if os_ else ds:.2e} sigma")
            elif os_ > 0:
                k = (entry, SC.path(n))
                if max(ds, db) / os_ > _worst.get(k, (-1.0,))[0]:
                    _worst[k] = (max(ds, db) / os_, what)
        elif not abs(gs - os_) <= WEAK_BAR * os_:
            bad.append(f"undecided case: sigma off by {abs(gs - os_) / os_:.2e} relative")
    if len(ref) > 2:
        if decided and got[2] != ref[2]:
            bad.append(f"nu {got[2]} where the oracle has {ref[2]}")
        elif not decided and got[2] not in SC.NU_GRID:
            bad.append(f"nu {got[2]} is no value of the bisection grid")
    for b in bad:
        fails.append(f"{entry} {what}: {b}; device {got}, oracle {ref}")


def none(fails):
    assert not fails, f"{len(fails)} misses:\n" + "\n".join(fails)


def report(n=None):
    for k, v in sorted(_worst.items()):
        print(f"worst device-vs-oracle deviation so far, {k[0]} / {k[1]}: {v[0]:.2e} sigma at {v[1]}")
    for k, v in sorted(_undecided.items()):
        print(f"undecided so far, {k}: {v[0]} of {v[1]}")


# ---- values ----------------------------------------------------------------------------------------------------------------------------------------

def array_results(ctx, make, n):
    """every array entry point on every case at n, the samples placed in device memory by make(e) -> {(entry, scale, contamination, mest): result}"""
    out = {}
    for s, c, e in SC.cases(n):
        d, s0 = make(e), SC.start_sigma(s)
        for mest in (SC.STUDENT, SC.HUBER):
            out[("student", s, c, mest)] = ctx.computeSigmaAndNuStudent(d, n, 0.0, s0, 5.0, mest)
        for mest in SC.MESTIMATORS:
            out[("pdf", s, c, mest)] = ctx.computeSigmaPdf(d, n, 0.0, s0, mest)
        out[("nu", s, c, SC.STUDENT)] = (ctx.computeNuStudent(d, n, SC.SCALES[s][1], SC.SCALES[s][0]),)
    return out


_exact = {}


def exact_results(ctx, n):
    if n not in _exact:
        _exact[n] = array_results(ctx, dev, n)
    return _exact[n]


@pytest.mark.parametrize("n", SC.COUNTS)
def test_sigma_nu_student_and_sigma_pdf_vs_oracle(ctx, n):
    """n = 1, 2, 3 run on seeds chosen on the CPU from the reference alone (sigma_cases.SEEDS): with two or three samples whose spread is a few per cent of
    their mean the reference's fp32 reduction swsr - 2 b swr + b^2 sw cancels to its last bits -- the oracle is then 1.7e-3 sigma from its own float64 mirror,
    and on such sets this kernel was measured 2.0e-3 sigma from the oracle (seed 0: n = 2 scale 1 clean; 1.0e-4 on n = 2 scale 2 tail, 3.3e-5 on n = 3
    scale 0 tail).  On the sets where the reference is pinned to 2e-6 the bar holds at these counts as at every other."""
    got, fails = exact_results(ctx, n), []
    for s, c, e in SC.cases(n):
        s0 = SC.start_sigma(s)
        for mest in (SC.STUDENT, SC.HUBER):
            ref = oracle_student(n, s, c, mest)
            hold(fails, "computeSigmaAndNuStudent", n, (n, s, c, mest), got[("student", s, c, mest)], ref, decided_student(n, s, c, mest))
            if c == "nan100":
                g = got[("student", s, c, mest)]
                assert np.isnan(g[0]) and np.isnan(g[1]) and g[2] == 9.75, g
        for mest in SC.MESTIMATORS:
            with np.errstate(all="ignore"):
                ref, dec = O.sigma_pdf(e, 0.0, s0, mest), SC.decided_pdf(e, s0, mest)
            hold(fails, f"computeSigmaPdf[{mest}]", n, (n, s, c, mest), got[("pdf", s, c, mest)], ref, dec)
            if c == "nan100":
                assert np.isnan(got[("pdf", s, c, mest)]).all()
        # computeNuStudent at the bias and scale the set was drawn with (tests/test_gpu_kfalign.py holds it at the aligner's counts and 1e30 outliers)
        nu, dec = SC.decided_nu(O.nu_student, e, SC.SCALES[s][1], SC.SCALES[s][0])
        u = _undecided.setdefault("computeNuStudent", [0, 0])
        u[0] += 0 if dec else 1
        u[1] += 1
        g = got[("nu", s, c, SC.STUDENT)][0]
        if (g != nu) if dec else (g not in SC.NU_GRID):
            fails.append(f"computeNuStudent {(n, s, c)}: nu {g} where the oracle has {nu} (decided: {dec})")
    report()
    none(fails)


@pytest.mark.parametrize("n", SC.COUNTS)
def test_chi_square_vs_oracle(ctx, n):
    worst = 0.0
    for c, ei, ed, si, sd in SC.chi_pairs(n):
        di, dd = dev(ei), dev(ed)
        for mest in SC.MESTIMATORS:
            x, t, cnt = ctx.computeChiSquare(di, dd, n, si, sd, mest)
            with np.errstate(all="ignore"):
                ox, ot, ocnt = O.chi_square(ei, ed, si, sd, mest)
            assert cnt == ocnt == np.isfinite(ei).sum() + np.isfinite(ed).sum(), (n, c, mest, cnt, ocnt)
            for g, o in ((x, ox), (t, ot)):
                if not np.isfinite(o):
                    assert SC.same_nonfinite(g, o), (n, c, mest, (x, t), (ox, ot))
            if np.isfinite(ox):
                worst = max(worst, abs(x - ox) / abs(ox))
                assert abs(x - ox) <= CHI_BAR * abs(ox), (n, c, mest, x, ox)
            if np.isfinite(ot):
                assert abs(t - ot) <= TAIL_BAR, (n, c, mest, t, ot)
    k = ("computeChiSquare", SC.path(n))
    if worst > _worst.get(k, (-1.0,))[0]:
        _worst[k] = (worst, n)
    print(f"n = {n}: chi-square worst {worst:.2e} relative")


def pair_lanes(n):
    """lanes of bt.sigma_pair: every contamination with the inverse-depth scale in channel 0 and each of the three intensity scales in channel 1"""
    return tuple((c, s1) for s1 in (1, 2, 3) for c in SC.CONTAMINATIONS)


def pair_host(n, lanes, stride=None, fill=POISON):
    stride = 2 * n if stride is None else stride
    res = np.full((len(lanes), stride), fill, np.float32)
    for l, (c, s1) in enumerate(lanes):
        res[l, :n] = SC.residuals(n, 0, c)
        res[l, n:2 * n] = SC.residuals(n, s1, c)
    return res


@pytest.mark.parametrize("n", SC.COUNTS)
def test_sigma_pair_vs_oracle(bt, n):
    lanes = pair_lanes(n)
    res, fails = dev(pair_host(n, lanes)), []
    for mest in (SC.STUDENT, SC.HUBER):
        out = bt.sigma_pair(res, n, mest)
        for l, (c, s1) in enumerate(lanes):
            for ch, s in ((0, 0), (1, s1)):
                got = tuple(out[l][k] for k in PAIR_KEYS[ch])
                hold(fails, "sigma_pair", n, (n, s, c, mest, "channel", ch), got, oracle_student(n, s, c, mest), decided_student(n, s, c, mest))
                if c == "nan100":
                    assert np.isnan(got[0]) and np.isnan(got[1]) and got[2] == 9.75, got
    report()
    none(fails)


# ---- nothing behind n is read ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SC.COUNTS)
def test_arrays_behind_n_are_not_read(ctx, n):
    """every array entry point with 1e30 in front of and behind the n samples: the bits of the exact-size array"""
    exact, pois = exact_results(ctx, n), array_results(ctx, poisoned, n)
    for k in exact:
        assert SC.bits(*pois[k]) == SC.bits(*exact[k]), (n, k, pois[k], exact[k])
    for c, ei, ed, si, sd in SC.chi_pairs(n):
        for mest in SC.MESTIMATORS:
            a = ctx.computeChiSquare(dev(ei), dev(ed), n, si, sd, mest)
            b = ctx.computeChiSquare(poisoned(ei), poisoned(ed), n, si, sd, mest)
            assert SC.bits(*a) == SC.bits(*b), (n, c, mest, a, b)


def pair_bits(out, chans=(0, 1)):
    return [tuple(SC.bits(*[o[k] for k in PAIR_KEYS[ch]]) for ch in chans) for o in out]


@pytest.mark.parametrize("n", SC.COUNTS)
def test_sigma_pair_gaps_and_the_other_channel_are_not_read(bt, n):
    """bt.sigma_pair with a lane stride of 2 n + 8 whose gap holds 1e30, and with 1e30 in the other channel's place: each channel's bits as with dense lanes"""
    lanes = pair_lanes(n)[:8]
    host = pair_host(n, lanes)
    dense = pair_bits(bt.sigma_pair(dev(host), n))
    gapped = dev(pair_host(n, lanes, stride=2 * n + 8))
    assert pair_bits(bt.sigma_pair(gapped, n)) == dense
    assert bool((gapped[:, 2 * n:] == float(POISON)).all())
    only0, only1 = host.copy(), host.copy()
    only0[:, n:] = POISON
    only1[:, :n] = POISON
    assert pair_bits(bt.sigma_pair(dev(only0), n), (0,)) == [d[:1] for d in dense]
    assert pair_bits(bt.sigma_pair(dev(only1), n), (1,)) == [d[1:] for d in dense]


# ---- lanes are independent ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ODD_COUNTS)
def test_lanes_are_independent(bt, n):
    """five lanes of different contaminations, an all-NaN lane in the middle, odd n (channel 1 of every lane and every second lane start 4-byte aligned
    only): each lane's bits are those of the same data run alone, and replacing a lane's neighbours leaves it alone"""
    lanes = (("clean", 1), ("wild", 2), ("nan100", 1), ("tail", 2), ("nan30", 1))
    host = pair_host(n, lanes, stride=2 * n + 8)
    batch = pair_bits(bt.sigma_pair(dev(host), n))
    for l in range(len(lanes)):
        alone = pair_bits(bt.sigma_pair(dev(host[l:l + 1, :2 * n]), n))
        assert alone[0] == batch[l], (n, l, lanes[l])
    other = host.copy()
    other[1], other[3] = host[3], host[1]
    other[2, :2 * n] = SC.residuals(2 * n, 1, "shift")
    swapped = pair_bits(bt.sigma_pair(dev(other), n))
    assert swapped[0] == batch[0] and swapped[4] == batch[4] and swapped[1] == batch[3] and swapped[3] == batch[1]


# ---- k_sigma_pair: the lattice through the getter's cursor ---------------------------------------------------------------------------------------------

# rows, cols, min_nsamples -> lattice columns: below 512 and no divisor of it; exactly 512; above 512 (the cursor's row advance is 0); 1 (its column
# advance is 0); a stride-2 lattice; 30 columns at stride 2 (no divisor either); more than 20 480 samples (the streaming path divides per sample)
MAP_GEOMS = [(61, 83, 9999999), (7, 512, 9999999), (5, 641, 9999999), (700, 1, 9999999), (48, 64, 500), (44, 60, 600), (145, 161, 9999999)]


def lattice_maps(rows, cols, stride, lane):
    """W1 - W0 and I1 - I0 carry a contaminated residual set on the lattice; off the lattice the first map of each pair holds 1e30"""
    r = np.random.default_rng([SC.SEED, rows, cols, lane])
    cont = ("nan30", "wild", "tail")[lane % 3]
    n = rows * cols
    W0 = r.uniform(0.25, 1.25, (rows, cols)).astype(np.float32)
    I0 = r.uniform(20.0, 235.0, (rows, cols)).astype(np.float32)
    W1 = (W0 + SC.residuals.__wrapped__(n, 0, cont, seed=100 + lane).reshape(rows, cols)).astype(np.float32)
    I1 = (I0 + SC.residuals.__wrapped__(n, 1 + lane % 2, cont, seed=100 + lane).reshape(rows, cols)).astype(np.float32)
    if stride > 1:
        off = np.ones((rows, cols), bool)
        off[::stride, ::stride] = False
        W1[off] = POISON
        I1[off] = POISON
    return W1, W0, I1, I0


def stack_padded(maps, pad):
    """[lanes, rows, cols] view of an allocation with `pad` more columns, those filled with 1e30"""
    a = np.stack(maps)
    big = np.full(a.shape[:2] + (a.shape[2] + pad,), POISON, np.float32)
    big[:, :, :a.shape[2]] = a
    return dev(big)[:, :, :a.shape[2]]


@pytest.mark.parametrize("rows,cols,ns", MAP_GEOMS)
def test_sigma_pair_maps_equals_sigma_pair_on_the_lattice(bt, rows, cols, ns):
    n, lr, lc, st = device.error_lattice_size(rows, cols, ns)
    lanes = 3
    L = [lattice_maps(rows, cols, st, l) for l in range(lanes)]
    dm = [stack_padded([m[i] for m in L], 3) for i in range(4)]
    res = np.empty((lanes, 2 * n), np.float32)
    for l, (W1, W0, I1, I0) in enumerate(L):
        ed, geo = O.error_lattice(W1, W0, ns)
        ei, _ = O.error_lattice(I1, I0, ns)
        assert ed.size == n and geo == (lr, lc, st) and np.abs(ed[np.isfinite(ed)]).max() < 1e3
        res[l, :n], res[l, n:] = ed, ei
    dres, fails = dev(res), []
    for mest in (SC.STUDENT, SC.HUBER):
        arrays, maps = bt.sigma_pair(dres, n, mest), bt.sigma_pair_maps(*dm, ns, mest)
        assert pair_bits(maps) == pair_bits(arrays), (rows, cols, ns, (lr, lc, st), maps, arrays)
        for l in range(lanes):
            for ch, s0 in ((0, 0.0025), (1, 5.0)):
                e = res[l, ch * n:(ch + 1) * n]
                with np.errstate(all="ignore"):
                    ref = O.sigma_nu_student(e, 0.0, s0, 5.0, mest)
                    dec = SC.decided_student(O.sigma_nu_student, e, s0, mest)[0]
                hold(fails, "sigma_pair_maps", n, (rows, cols, ns, l, ch, mest), tuple(maps[l][k] for k in PAIR_KEYS[ch]), ref, dec)
    report()
    none(fails)


def test_sigma_pair_maps_refuses_what_its_siblings_refuse(bt):
    import ctypes as C
    from rgbid._lib import RgbidError
    a = dev(np.zeros((2, 8, 16), np.float32)); b = dev(np.zeros((2, 8, 12), np.float32))
    with pytest.raises(RgbidError):
        bt.sigma_pair_maps(a, a, a, b, 100)
    with pytest.raises(RgbidError):
        bt.sigma_pair_maps(a, a, a, a, 100, mestimator=4)
    out, ms = (BT.ScalePair * 2)(), C.c_float()
    bad = BT.imgb(a); bad.step = 4 * 16 - 4
    assert bt.L.rgbid_sigma_pair_maps_batched(bt._h, 2, C.byref(BT.imgb(a)), C.byref(bad), C.byref(BT.imgb(a)), C.byref(BT.imgb(a)), 100, 3, out, C.byref(ms)) == -1
    assert bt.L.rgbid_sigma_pair_maps_batched(bt._h, 2, C.byref(BT.imgb(a)), C.byref(BT.imgb(a)), C.byref(BT.imgb(a)), C.byref(BT.imgb(a)), 100, 3, None, C.byref(ms)) == -1
