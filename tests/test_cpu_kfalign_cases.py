"""The condition that keeps tests/test_gpu_kfalign.py honest (CPU test, no GPU needed): on every pair of tests/kfalign_cases.py that the GPU test holds
to 1e-4 rad / 1e-4 m / 1e-2 of O.keyframe_align, the oracle itself is finite and well conditioned -- its IEEE build and the build that models the
reference's nvcc numerics (librgbid_oracle_cudanum.so) agree to a TENTH of that bar.  The device code is one more set of numerics of the same kind
(reciprocals, FMA contraction, another summation order); where two of them differ by 1e-5 a third cannot be asked for 1e-4 with a straight face.

Seeds: tests/kfalign_cases.py SEEDS lists the pairs whose first seed missed this (a third of the small-size seeds do: a nu bisection step on a
few thousand samples flips with the last bit).  The 32x32 `unrelated` pair of the issue's table (3.6e-5 rad between the builds) got ANOTHER SEED and stays
`unrelated`; the 32x32 `photometric_only` pair is MOVED TO `wild`: it is ill-conditioned at every seed (kfalign_cases.WILD_CELLS has the figures).
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import kfalign_cases as KC

needs_fma = pytest.mark.skipif(not O.cpu_has_fma(), reason="LOUD SKIP: librgbid_oracle_cudanum.so needs a host CPU with FMA (-mfma)")

ALL_SIZES = KC.SIZES + [KC.MANY_PAIRS_SIZE]
# a tenth of the bar of the GPU test.  Measured over the corpus (worst cell): 3.2e-6 rad, 3.1e-6 m, 6.1e-5 covariance
SPREAD_ROT, SPREAD_TRANS, SPREAD_COV = 1e-5, 1e-5, 1e-3
# tests/test_gpu_tracker_cpp.py::test_keyframe_align_batched: the true relative pose.  Measured (worst cell, `shifted` at 32x32, where one pixel is 0.038 rad):
# 1.9e-3 rad, 3.6e-3 m
TRUTH_ROT, TRUTH_TRANS = 4e-3, 1.5e-2


def _align(c, **kw):
    return O.keyframe_align(c.iD_ini, c.grey_ini, c.iD_end, c.grey_end, c.K, R0=c.R0, t0=c.t0, **kw)


def _blind(res):
    """A = 0: R and t are NaN throughout, as Eigen's LLT of a zero matrix leaves them, and the covariance holds no finite entry (the inverse's last
    pivot is 1 / 0 = inf, every other entry NaN)"""
    return np.isnan(res[0]).all() and np.isnan(res[1]).all() and not np.isfinite(res[2]).any()


def _finite(res):
    return all(np.isfinite(x).all() for x in res)


def test_corpus_is_what_it_says():
    """the corpus itself: every size has every pair, the kinds are the documented ones, the holes are there, builds are reproducible"""
    for rows, cols in ALL_SIZES:
        cs = KC.cases(rows, cols)
        assert [c.name for c in cs] == list(KC.NAMES)
        by = {c.name: c for c in cs}
        for c in cs:
            assert c.iD_ini.shape == c.iD_end.shape == c.grey_ini.shape == c.grey_end.shape == (rows, cols)
            assert c.iD_ini.dtype == np.float32 and c.grey_ini.dtype == np.uint8
            expect = "wild" if c.name in ("turned", "blind", "nan_guess") or ((rows, cols), c.name) in KC.WILD_CELLS else "unrelated" if c.name == "unrelated" else "posed"
            assert c.kind == expect, (rows, cols, c.name)
            assert (c.truth is not None) == (c.name in ("same_holes", "shifted", "photometric_only", "perturbed_rotation"))
        h = np.isnan(by["same_holes"].iD_ini).mean(), np.isnan(by["same_holes"].iD_end).mean()
        assert 0.18 < h[0] < 0.32 and h[0] < h[1] < 0.42, h                           # 25 % holes, 10 % more in the second keyframe
        assert np.isnan(by["shifted"].iD_end[:, cols - cols // 8:]).all()             # the cropped border
        assert np.isnan(by["photometric_only"].iD_end).all() and np.isnan(by["blind"].iD_ini).all()
        assert np.isnan(by["nan_guess"].R0).sum() == 1 and KC.rot_angle(by["turned"].R0, np.eye(3)) == pytest.approx(np.pi)
        assert not np.array_equal(by["unrelated"].grey_ini, by["unrelated"].grey_end)
        again = KC.case.__wrapped__("shifted", rows, cols)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(again[1:5], by["shifted"][1:5]))


def test_rendered_view_is_the_scene_under_the_motion():
    """Scene.view solves for the surface along each ray: the point it finds projects into the scene camera where the depth function has that depth"""
    rows, cols = 61, 83
    K = KC.intrinsics(rows, cols)
    S = KC.Scene(rows, cols, 3)
    R, t = KC.rot((0.2, 1.0, -0.1), np.deg2rad(1.0)), np.array([0.012, -0.006, 0.007])
    w, g, inside = S.view(K, R, t)
    v, u = np.mgrid[0:rows, 0:cols].astype(np.float64)
    X = (np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones_like(u)], -1) / w[..., None]) @ R.T + t
    x1, y1 = K[0] * X[..., 0] / X[..., 2] + K[2], K[1] * X[..., 1] / X[..., 2] + K[3]
    assert np.abs(S.depth(x1, y1) - X[..., 2]).max() < 1e-12
    assert np.abs(S.grey(x1, y1) - g).max() < 1e-9
    assert 0.5 < inside.mean() < 1.0
    w0, g0, _ = S.view(K)
    wi, gi, ii = S.view(K, np.eye(3), np.zeros(3))
    assert np.abs(w0 - wi).max() < 1e-15 and np.abs(g0 - gi).max() < 1e-9 and ii.all()


@pytest.mark.parametrize("rows,cols", ALL_SIZES)
def test_oracle_is_finite_and_finds_the_motion(rows, cols):
    worst = [0.0, 0.0]
    for c in KC.cases(rows, cols):
        res = _align(c)
        if c.kind == "wild":
            if c.name == "blind":
                assert _blind(res), c.name
            continue
        assert _finite(res), (rows, cols, c.name)
        if c.truth is not None:
            dr, dt = KC.rot_angle(res[0], c.truth[0]), float(np.linalg.norm(res[1] - c.truth[1]))
            print(f"{rows}x{cols} {c.name}: {dr:.2e} rad, {dt:.2e} m from the true motion")
            worst = [max(worst[0], dr), max(worst[1], dt)]
            assert dr < TRUTH_ROT and dt < TRUTH_TRANS, (rows, cols, c.name, dr, dt)
    print(f"{rows}x{cols}: worst distance from the true motion {worst[0]:.2e} rad, {worst[1]:.2e} m")


@needs_fma
@pytest.mark.parametrize("rows,cols", ALL_SIZES)
def test_oracle_builds_agree_to_a_tenth_of_the_bar(rows, cols):
    worst = {}
    for c in KC.cases(rows, cols):
        a, b = _align(c), _align(c, numerics="cuda")
        d = KC.deviation(a, b)
        print(f"{rows}x{cols} {c.name} ({c.kind}): builds differ by {d[0]:.2e} rad, {d[1]:.2e} m, {d[2]:.2e} covariance")
        if c.kind == "wild":
            if c.name == "blind":
                assert _blind(b)
            continue
        assert _finite(b), (rows, cols, c.name)
        assert d[0] < SPREAD_ROT and d[1] < SPREAD_TRANS and d[2] < SPREAD_COV, (rows, cols, c.name, d)
        w = worst.setdefault(c.kind, [0.0, 0.0, 0.0])
        worst[c.kind] = [max(x, y) for x, y in zip(w, d)]
    for kind, w in worst.items():
        print(f"{rows}x{cols} worst spread of the builds, {kind}: {w[0]:.2e} rad, {w[1]:.2e} m, {w[2]:.2e} covariance")


@needs_fma
def test_exact_interpolation_is_as_well_conditioned():
    """the pairs the GPU test aligns with INTERP_EXACT (61x83)"""
    for c in KC.cases(61, 83):
        if c.kind == "wild":
            continue
        a, b = _align(c, interp_mode=O.INTERP_EXACT), _align(c, interp_mode=O.INTERP_EXACT, numerics="cuda")
        d = KC.deviation(a, b)
        print(f"61x83 {c.name} INTERP_EXACT: builds differ by {d[0]:.2e} rad, {d[1]:.2e} m, {d[2]:.2e} covariance")
        assert _finite(a) and d[0] < SPREAD_ROT and d[1] < SPREAD_TRANS and d[2] < SPREAD_COV, (c.name, d)
        assert not np.array_equal(a[1], _align(c)[1])     # and the mode does change the result


def test_nu_cases_are_decided_in_the_oracle():
    """the residual sets of the GPU nu test: at most one in ten may sit on a bisection step (kfalign_cases.nu_decided); all-NaN and overflowing sets have
    the values the reference's arithmetic gives them"""
    undecided = []
    for n in KC.NU_COUNTS:
        for cont in KC.NU_CONTAMINATIONS:
            with np.errstate(over="ignore", invalid="ignore"):
                nu, dec = KC.nu_decided(O.nu_student, KC.nu_residuals(n, cont))
            assert 2.0 <= nu <= 10.0 and nu * 4 == int(nu * 4)
            if not dec:
                undecided.append((n, cont))
            if cont == "nan100":
                assert nu == 9.75 and dec      # 0 / 0: every comparison of the bisection is false
            if cont == "huge":
                assert nu == 2.0 and dec       # en^2 = inf: ln w = -inf at every nu
    # the wide tail decides nu: without the samples beyond the 20 480 a workgroup's registers hold, the answer is another one
    e = KC.nu_residuals(23345, "tail")
    assert O.nu_student(e, KC.NU_BIAS, KC.NU_SIGMA) != O.nu_student(e[:20480], KC.NU_BIAS, KC.NU_SIGMA)
    total = len(KC.NU_COUNTS) * len(KC.NU_CONTAMINATIONS)
    print(f"undecided nu cases in the oracle: {len(undecided)} of {total}: {undecided}")
    assert 10 * len(undecided) <= total


def test_verdict_keyframes_keep_the_oracle_away_from_the_gate():
    """the keyframes of the GPU test of loop_constraints: the oracle accepts the second view, rejects the unrelated scene by the gate and the keyframe
    without depth as not finite, every finite correction sits ten bars (1e-3) or more from the gate, and the builds agree as everywhere else"""
    K = KC.intrinsics(*KC.VERDICT_SIZE)
    kfs, guess = KC.verdict_keyframes()
    verdicts = []
    for (q, c), (R0, t0) in zip(KC.VERDICT_PAIRS, guess):
        a = O.keyframe_align(kfs[q][0], kfs[q][1], kfs[c][0], kfs[c][1], K, R0=R0, t0=t0)
        ok, corr = KC.verdict(*a, R0, t0)
        print(f"pair {(q, c)}: accepted {ok}, correction {corr[0]:.4e} m, {corr[1]:.4e} rad")
        verdicts.append(ok)
        if np.isfinite(corr[0]):
            assert abs(corr[0] - 0.1) >= 1e-3 and abs(corr[1] - 0.1) >= 1e-3
            if O.cpu_has_fma():
                b = O.keyframe_align(kfs[q][0], kfs[q][1], kfs[c][0], kfs[c][1], K, R0=R0, t0=t0, numerics="cuda")
                d = KC.deviation(a, b)
                print(f"pair {(q, c)}: builds differ by {d[0]:.2e} rad, {d[1]:.2e} m, {d[2]:.2e} covariance")
                assert d[0] < SPREAD_ROT and d[1] < SPREAD_TRANS and d[2] < SPREAD_COV
    assert verdicts == [True, False, False]
