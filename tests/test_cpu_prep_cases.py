"""Pins the reference on the frame-preparation cases (tests/prep_cases.py) before the GPU is held to it: the C oracle against the float64 mirror
(tests/np_mirror.py) on EVERY case, validity patterns equal without exception, values within twice the worst deviation measured over the full case set
(the figures are in DESIGN.md 7.2 and in BARS below) -- and the properties that make the cases mean something: count cases with exactly 12 / 13 valid taps,
sparse cases with invalid and valid outputs, keyframe maps on both sides of the normal gate.  No GPU."""
import numpy as np

from oracle import oracle as O
from tests import np_mirror as M
from tests import prep_cases as P

# worst oracle-vs-mirror deviation over the full case set (measured; printed by every test), the bar is twice that
MEASURED = {"pyr": 5.87e-7, "bilateral": 5.87e-7, "sobel": 2.13e-6, "sobel_magnitude": 5.25e-8, "depth2invdepth": 1.35e-7, "intensity": 9.3e-8, "vmap": 3.03e-7,
            "nmap": 1.86e-7}
BARS = {k: 2 * v for k, v in MEASURED.items()}
# Beyond 2e-6 the oracle itself needs a look first.  One figure is: the Sobel error RELATIVE TO THE MAP'S RANGE reaches 2.1e-6 -- on the 4 x 1 and 65 x 1
# inverse-depth maps, whose range (0.0035 .. 0.016) is under 3 % of their magnitude (0.5).  The error there is 1.5e-8 .. 4.4e-8 of the magnitude, a fraction of
# an fp32 ulp of the taps the oracle adds: it is the yardstick that shrinks, not the oracle that drifts.  Relative to the largest magnitude the worst case of
# the whole set is 5.2e-8; both are asserted.
assert max(v for k, v in BARS.items() if k != "sobel") < 2e-6


def _rel(got, ref, scale=None):
    """-> worst |got - ref| / scale over the pixels both define (scale: |ref| unless given); validity must be EQUAL"""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    ng, nr = np.isnan(got), np.isnan(ref)
    assert np.array_equal(ng, nr), f"validity differs at {np.count_nonzero(ng != nr)} pixels"
    m = ~nr
    if not m.any():
        return 0.0
    s = np.abs(ref[m]) if scale is None else scale
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.abs(got[m] - ref[m]) / s
    q = np.where(got[m] == ref[m], 0.0, q)
    return float(q.max())


def _all_float_cases(kind):
    whiches = ("W", "I") if kind != "sobelfb" else ("W",)
    return [c for w in whiches for c in P.float_cases(kind, w)]


def test_pyramid_oracle_against_mirror():
    worst, n = 0.0, 0
    for c in _all_float_cases("pyr"):
        with np.errstate(all="ignore"):
            worst = max(worst, _rel(O.pyr_down(c.map), M.pyr_down(c.map))); n += 1
    print(f"pyrDown: {n} cases, worst relative {worst:.2e} (bar {BARS['pyr']:.1e})")
    assert n > 1000 and worst <= BARS["pyr"], worst


def test_bilateral_oracle_against_mirror():
    worst, n = 0.0, 0
    for kind, sigmas in (("bil_fast", P.FAST_SIGMAS), ("bil_fast32", P.FAST_SIGMAS), ("bil_exact", P.EXACT_SIGMAS)):
        for which, sigma in sigmas:
            for c in P.float_cases(kind, which):
                a = P.sanitised(c.map)
                with np.errstate(all="ignore"):
                    worst = max(worst, _rel(O.bilateral(a, sigma), M.bilateral(a, sigma))); n += 1
    print(f"bilateral: {n} cases, worst relative {worst:.2e} (bar {BARS['bilateral']:.1e})")
    assert n > 1000 and worst <= BARS["bilateral"], worst


def _range_and_magnitude(a):
    v = a[~np.isnan(a)]
    if not v.size:
        return 1.0, 1.0
    mag = float(np.abs(v).max())
    return max(float(v.max() - v.min()), 1e-3 * mag), mag


def test_sobel_oracle_against_mirror():
    worst, worst_mag, n = 0.0, 0.0, 0
    for c in _all_float_cases("sobel16") + _all_float_cases("sobelfb"):
        rng_, mag = _range_and_magnitude(c.map)
        with np.errstate(all="ignore"):
            for g, m in zip(O.gradient(c.map), M.sobel(c.map)):
                e = _rel(g, m, 1.0)
                worst, worst_mag = max(worst, e / rng_), max(worst_mag, e / mag)
        n += 1
    print(f"Sobel: {n} cases, worst error relative to the map's range {worst:.2e} (bar {BARS['sobel']:.1e}), to its largest magnitude {worst_mag:.2e} "
          f"(bar {BARS['sobel_magnitude']:.1e})")
    assert n > 500 and worst <= BARS["sobel"] and worst_mag <= BARS["sobel_magnitude"], (worst, worst_mag)


def test_converters_oracle_against_mirror():
    wd = wi = 0.0
    for c in P.prep_cases():
        assert set(P.PREP_DEPTHS) <= set(c.depth.reshape(-1).tolist())
        assert all(c.rgb[..., k].min() == 0 and c.rgb[..., k].max() == 255 for k in range(3))
        for factor in (1.0, 0.96):
            wd = max(wd, _rel(O.depth2invdepth(c.depth, factor), M.depth_to_invdepth(c.depth, factor)))
        wi = max(wi, _rel(O.intensity(c.rgb), M.intensity(c.rgb), 255.0))
        for got, k in zip(O.decompose_rgb(c.rgb), range(3)):
            assert np.array_equal(got, c.rgb[..., k].astype(np.float32))
    print(f"converters: depth2invdepth worst relative {wd:.2e} (bar {BARS['depth2invdepth']:.1e}), intensity worst / 255 {wi:.2e} (bar {BARS['intensity']:.1e})")
    assert wd <= BARS["depth2invdepth"] and wi <= BARS["intensity"]
    # the clamp: 10 000, 10 001 and 65 535 mm are all 0.1 m^-1, 9 999 is not; 0 is invalid
    o = O.depth2invdepth(np.array([P.PREP_DEPTHS], np.uint16))[0]
    assert np.isnan(o[0]) and o[1] == 1000.0 and o[2] > o[3] and o[3] == o[4] == o[5] == np.float32(0.1)


def test_keyframe_maps_oracle_against_mirror():
    wv = wn = 0.0
    n = 0
    for c in P.kf_cases():
        K = c.meta
        with np.errstate(all="ignore"):
            ov, mv = O.vmap(c.map, K), M.vmap(c.map, K)
            gx, gy = O.gradient(c.map)
            on, mn = O.nmap_gradients(c.map, gx, gy, K), M.nmap_gradients(c.map, gx, gy, K)
        rows = c.rows
        valid = ~np.isnan(c.map)
        assert np.array_equal(~np.isnan(ov[:rows]), valid)
        zmax = float(np.abs(mv[2][valid]).max()) if valid.any() else 1.0
        for p in range(3):
            got, ref = ov[p * rows:(p + 1) * rows].copy(), mv[p].copy()
            got[~valid] = np.nan; ref[~valid] = np.nan      # planes 1 / 2 of an invalid pixel: the reference leaves them untouched
            wv = max(wv, _rel(got, ref, zmax))
        nvalid = ~np.isnan(on[:rows])
        for p in range(3):
            got, ref = on[p * rows:(p + 1) * rows].copy(), mn[p].copy()
            got[~nvalid] = np.nan
            wn = max(wn, _rel(got, ref, 1.0))               # unit vectors: absolute = relative to the norm
        if c.content != "allnan":
            passed, rejected = P.kf_gate_sides(c.map, K)
            assert passed > 0 and rejected > 0, (c.name, passed, rejected)
            defined = ~(np.isnan(c.map) | np.isnan(gx) | np.isnan(gy))
            assert np.count_nonzero(defined & nvalid) > 0 and np.count_nonzero(defined & ~nvalid) > 0, c.name     # ... and so says the oracle
        n += 1
    print(f"keyframe maps: {n} cases, vertex worst / max depth {wv:.2e} (bar {BARS['vmap']:.1e}), normal worst absolute {wn:.2e} (bar {BARS['nmap']:.1e})")
    assert wv <= BARS["vmap"] and wn <= BARS["nmap"]


def test_count_cases_have_exactly_12_and_13_valid_taps():
    for c in P.float_cases("pyr"):
        if c.content != "count":
            continue
        n = P.valid_taps(c.map)
        ref = O.pyr_down(c.map)
        seen = set()
        for y, x, k in c.meta:
            assert k in (12, 13) and n[y, x] == k, (c.name, y, x, k, int(n[y, x]))
            assert np.isnan(ref[y, x]) == (k == 12), (c.name, y, x, k)        # `count > 12`
            interior = 2 * y - 2 >= 0 and 2 * x - 2 >= 0
            seen.add((k, interior))
        assert seen == {(12, True), (13, True), (12, False), (13, False)}, (c.name, seen)
        assert len(c.meta) >= 14, (c.name, len(c.meta))       # each of the seven layouts and its complement
    assert sum(c.content == "count" for c in P.float_cases("pyr")) == len(P.COUNT_SHAPES)


# sources so small that no window holds 13 taps: every output is invalid whatever the content
PYR_NO_VALID_OUTPUT = {(2, 2), (2, 3), (3, 2), (2, 130)}


def test_sparse_cases_have_invalid_and_valid_outputs():
    n = 0
    for kind, fn in (("pyr", O.pyr_down), ("bil_fast", lambda a: O.bilateral(a, 3.0)), ("bil_fast32", lambda a: O.bilateral(a, 3.0)),
                     ("bil_exact", lambda a: O.bilateral(a, 3.0)), ("sobel16", lambda a: O.gradient(a)[0]), ("sobelfb", lambda a: O.gradient(a)[0])):
        for c in P.float_cases(kind, "I" if kind != "sobelfb" else "W"):
            if c.content != "sparse":
                continue
            assert np.count_nonzero(np.isnan(c.map)) == 1 and np.isnan(c.map[c.meta])
            out = fn(c.map)
            if kind == "pyr" and (c.rows, c.cols) in PYR_NO_VALID_OUTPUT:
                assert np.isnan(out).all()
                continue
            assert np.isnan(out).any() and (~np.isnan(out)).any(), c.name
            n += 1
    assert n > 1000
    # the single hole of a pyramid case never invalidates an output (24 of 25 taps): it is the fast path that it switches off
    for c in P.float_cases("pyr"):
        if c.content == "sparse":
            clean = next(k for k in P.float_cases("pyr") if (k.rows, k.cols, k.content) == (c.rows, c.cols, "clean"))
            assert np.array_equal(np.isnan(O.pyr_down(c.map)), np.isnan(O.pyr_down(clean.map)))


def test_the_shapes_of_the_issue_are_all_there():
    s = P.SHAPES
    assert {c for _, c in s["pyr"]} >= {122, 123, 124, 125, 126, 127, 248, 249, 250, 251} and {r for r, _ in s["pyr"]} >= {14, 15, 16, 17, 18, 19, 32, 33, 34, 35}
    assert {(2, 2), (2, 3), (3, 2), (4, 4), (5, 5), (2, 130)} <= set(s["pyr"])
    assert {c for _, c in s["bil_fast"]} >= {1, 2, 3, 59, 60, 61, 119, 120, 121, 181}
    assert {r for r, _ in s["bil_fast"]} >= {1, 2, 3, 4, 5, 29, 30, 31, 32, 33, 59, 60, 61, 119, 120, 121} and {(480, 120), (480, 121)} <= set(s["bil_fast"])
    assert {r for r, _ in s["bil_fast32"]} == {59, 60, 61, 62, 239, 240, 241}
    assert {c for _, c in s["bil_exact"]} >= {1, 63, 64, 65, 127, 128, 129} and {r for r, _ in s["bil_exact"]} >= {1, 15, 16, 17, 31, 32, 33} and (64, 128) in s["bil_exact"]
    assert {c for _, c in s["sobel16"]} == {4, 8, 60, 64, 68, 256} and {r for r, _ in s["sobel16"]} >= {1, 2, 7, 8, 9, 15, 16, 17, 121, 128, 129}
    assert all(c % 4 == 0 for _, c in s["sobel16"]) and all(c % 4 for _, c in s["sobelfb"])
    assert {c for _, c in s["sobelfb"]} == {1, 2, 3, 63, 65, 66, 129} and {r for r, _ in s["sobelfb"]} >= {1, 3, 4, 5, 63, 64, 65}
    units = sorted(r * (c // 4) for r, c in P.PREP_SHAPES if c % 4 == 0)
    assert {511, 512, 513, 1024, 1025} <= set(units) and any(c % 4 for _, c in P.PREP_SHAPES)
