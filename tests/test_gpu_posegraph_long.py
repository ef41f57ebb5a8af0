"""GPU tests of the envelope reduced-system solver (rgbid_pg_set_limits): graphs with more than RGBID_PG_MAX_SEPARATORS separators, byte
equality with the dense solver below the cap, the float64 mirror (tests/pg_mirror.py) above it."""
import numpy as np
import pytest

from rgbid import posegraph as PG
from rgbid._lib import RgbidError
from tests import pg_mirror as M
from tests.pg_mirror import comb as _comb, pose_err as _pose_err

pytestmark = pytest.mark.gpu

E_INVALID = -1


def _batch(seed, n):
    r = np.random.default_rng(seed)
    graphs = []
    for g in range(n):
        T = int(r.integers(5, 120))
        lost = tuple(int(x) for x in r.integers(1, T, size=int(r.integers(0, 3))))
        graphs.append(M.make_graph(r, T, K=int(r.integers(2, 12)), L=int(r.integers(0, 4)), lost=lost, drift=0.005, noise=1e-4)[:2])
    return graphs


def _separators(P, E, stage):
    return len(PG.envelope(len(P), E, stage)[0])


def _long_graph():
    P, E, GT = M.make_graph(np.random.default_rng(7), 1200, K=400, L=12, drift=0.005, noise=1e-4)
    return P, E


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_envelope_equals_dense_bytewise(ctx):
    """every graph the dense solver takes: set_limits(256, 1) (envelope always) returns the bytes of a default solver (dense)"""
    r = np.random.default_rng(5)
    target = M.make_graph(r, 150, K=12, L=4, lost=(40,), drift=0.01, noise=1e-4)[:2]
    small = [M.make_graph(r, int(r.integers(3, 12)), K=3, L=1)[:2] for _ in range(16)]
    big = [small[k % 16] for k in range(2047)]
    big.insert(1234, target)
    sets = [("random 12", _batch(12, 24)), ("random 11", _batch(11, 24)), ("target", [target]), ("batch of 2048", big), ("comb 256", [_comb(PG.MAX_SEPARATORS)])]
    dense, env = PG.PoseGraph(ctx), PG.PoseGraph(ctx)
    try:
        env.set_limits(PG.MAX_SEPARATORS, 1)
        for name, graphs in sets:
            for ml in (True, False):
                for iters in (None, (1, 0, 1), (2, 1, 2)):
                    a = dense.optimise(graphs, multilevel=ml, iters=iters)
                    b = env.optimise(graphs, multilevel=ml, iters=iters)
                    assert (a[1] == PG.OK).all(), (name, ml, iters)
                    assert _same(a, b), (name, ml, iters)
    finally:
        dense.close()
        env.close()


@pytest.mark.parametrize("multilevel", [True, False])
@pytest.mark.parametrize("iters", [(1, 0, 1), (2, 1, 2), None])
def test_above_the_cap_matches_mirror(ctx, multilevel, iters):
    """358 separators (> 256): refused by a default solver, solved after set_limits; each truncated step within 1e-9 m / 1e-9 rad of the
    mirror, the full schedule within 1e-7, chi2 as in test_random_batches_match_mirror.
    Measured on an MI355X (m / rad): (1, 0, 1) 1.2e-12 / 9.1e-14 multilevel and 3.2e-12 / 2.2e-13 single level, (2, 1, 2) 3.6e-14 / 3.1e-15
    and 3.5e-14 / 3.4e-15, full schedule 5.3e-15 / 5.9e-16 and 7.1e-15 / 6.9e-16."""
    P, E = _long_graph()
    ns = _separators(P, E, 0 if multilevel else 2)
    assert ns > PG.MAX_SEPARATORS, ns
    pg = PG.PoseGraph(ctx)
    try:
        with pytest.raises(RgbidError):
            pg.optimise([(P, E)], multilevel=multilevel, iters=iters)
        pg.set_limits(len(P))
        out, status, chi2 = pg.optimise([(P, E)], multilevel=multilevel, iters=iters)
    finally:
        pg.close()
    assert status[0] == PG.OK
    ref = M.optimise(P, E, multilevel=multilevel, **({} if iters is None else dict(iters=iters)))
    dt, ang = _pose_err(out[0], ref)
    print(f"{ns} separators, iters {iters} {'multilevel' if multilevel else 'single level'}: max deviation {dt:.3e} m, {ang:.3e} rad")
    bound = 1e-7 if iters is None else 1e-9
    assert dt <= bound and ang <= bound, (dt, ang)
    assert float(np.abs(ref - P).max()) > 1e-4
    E0, E1 = (E[E["type"] != PG.SEQ_ODO], E[E["type"] == PG.SEQ_ODO]) if multilevel else (E, E)
    assert chi2[0, 0] == pytest.approx(M.chi2(P, E0), rel=1e-9)
    assert chi2[0, 1] == pytest.approx(M.chi2(out[0], E1), rel=1e-6, abs=1e-9)


def _records(F):
    from rgbid.dist import GATHER_DTYPE
    r = np.zeros(F, GATHER_DTYPE)
    for j in range(F):
        r[j]["frame_id"] = j
        r[j]["R"] = np.eye(3)
        r[j]["t"] = [0.01, 0.0, 0.0] if j else [0.0, 0.0, 0.0]
        r[j]["cov"] = 1e-4 * np.eye(6) if j else np.zeros((6, 6))
    return r


@pytest.mark.parametrize("mode", ["multilevel", "single"])
def test_optimise_run_with_more_than_256_keyframes(ctx, mode):
    """a run of 640 frames that exported 319 keyframes (one every second frame): optimise_run raises the limit itself"""
    F = 640
    rng = np.random.default_rng(3)
    R = np.tile(np.eye(3), (F, 1, 1))
    t = np.zeros((F, 3))
    t[:, 0] = 0.01 * np.arange(F)
    t += np.cumsum(rng.normal(0, 2e-4, (F, 3)), 0)                  # the composed trajectory drifted off its own measurements
    t[0] = 0
    hdr = [(0, dict(id=k, end_id=k + 2, R_rel=np.eye(3), t_rel=np.array([0.02, 0.0, 0.0]), cov_rel=np.eye(6) * 1e-4)) for k in range(0, F - 2, 2)]
    assert len(hdr) > PG.MAX_SEPARATORS
    Ro, to, info = PG.optimise_run(ctx, R, t, [_records(F)], [0], hdr, None, None, optimise=mode)
    assert info["mode"] == mode and info["status"] == PG.OK
    P, E = PG.graph_from_run(R, t, [_records(F)], [0], hdr)
    assert _separators(P, E, 0 if mode == "multilevel" else 2) > PG.MAX_SEPARATORS
    # every measurement says 0.01 m per frame along x: the optimum is the straight line
    line = np.zeros((F, 3))
    line[:, 0] = 0.01 * np.arange(F)
    print(f"optimise_run {mode}: chi2 {info['chi2'][0]:.3e} -> {info['chi2'][1]:.3e}, off the line before {np.abs(t - line).max():.3e} m, after {np.abs(to - line).max():.3e} m")
    assert np.abs(to - line).max() <= 1e-9 and np.abs(Ro - np.eye(3)).max() <= 1e-9
    pg = PG.PoseGraph(ctx)
    try:
        pg.set_limits(F)
        out, _, _ = pg.optimise([(P, E)], multilevel=mode == "multilevel")
    finally:
        pg.close()
    assert np.array_equal(out[0][:, 9:], to)


def test_far_above_the_cap(ctx):
    """5 400 keyframes over 12 000 frames (about 4 300 of them separators: a keyframe between two neighbouring keyframes is none) with loops
    back to keyframe 0, and a comb of 4 097 separators"""
    # Gauss-Newton has no damping: it needs the start inside its basin.  The accumulated rotation drift of the start is drift * sqrt(T); the
    # drift is scaled so that it equals that of test_loops_remove_drift (0.005 at T = 300: 0.087 rad).  With 0.005 at T = 12 000 (0.55 rad,
    # ATE 50 m) ten iterations only reach 6.3 m, and the float64 mirror shows the same on a graph of a tenth the size with the same 0.55 rad
    # (ATE 8.07 m -> 0.061 m, against 1.24 m -> 1.7e-4 m at 0.087 rad): that is the schedule, not the solver
    T = 12000
    P, E, GT = M.make_graph(np.random.default_rng(41), T, K=5400, L=64, drift=0.005 * np.sqrt(300 / T), noise=1e-5, loops_to_start=True)
    r = np.random.default_rng(6)
    small = [M.make_graph(r, int(r.integers(3, 40)), K=3, L=1)[:2] for _ in range(8)]
    ate = lambda X: float(np.sqrt(np.mean(np.sum((X[:, 9:] - GT[:, 9:]) ** 2, 1))))
    pg = PG.PoseGraph(ctx)
    try:
        pg.set_limits(len(P))
        for ml in (True, False):
            ns = _separators(P, E, 0 if ml else 2)
            assert ns >= 4096, ns
            a = pg.optimise([(P, E)], multilevel=ml)
            before, after = ate(P), ate(a[0][0])
            print(f"{ns} separators ({'multilevel' if ml else 'single level'}): ATE before {before:.4f} m, after {after:.3e} m ({after / before:.2e} of it); "
                  f"chi2 {a[2][0, 0]:.3e} -> {a[2][0, 1]:.3e}")
            assert a[1][0] == PG.OK
            assert after < 1e-2 * before
            b = pg.optimise([(P, E)], multilevel=ml)
            assert _same(a, b)
            batch = small[:5] + [(P, E)] + small[5:]
            c = pg.optimise(batch, multilevel=ml)
            assert (c[1] == PG.OK).all()
            assert np.array_equal(c[0][5], a[0][0]) and np.array_equal(c[2][5], a[2][0])
        Pm, many = _comb(4097)
        default = PG.PoseGraph(ctx)
        try:
            with pytest.raises(RgbidError):
                default.optimise([(Pm, many)], multilevel=True)
        finally:
            default.close()
        out, status, chi2 = pg.optimise([(Pm, many)], multilevel=True, iters=(2, 0, 0))
        assert status[0] == PG.OK and np.isfinite(out[0]).all()
        c0, c1 = M.chi2(Pm, many), M.chi2(out[0], many)
        print(f"comb of 4097 separators: chi2 {c0:.6e} -> {c1:.6e}")
        assert chi2[0, 0] == pytest.approx(c0, rel=1e-9) and c1 < c0
    finally:
        pg.close()


def test_mixed_batch_equals_solo(ctx):
    """dense-path graphs and envelope-path graphs in one call: each result is its solo result"""
    long1 = _long_graph()
    long2 = M.make_graph(np.random.default_rng(8), 900, K=300, L=5, drift=0.005, noise=1e-4)[:2]
    smalls = _batch(17, 6)
    batch = smalls[:2] + [long1] + smalls[2:5] + [long2] + smalls[5:]
    pg, default = PG.PoseGraph(ctx), PG.PoseGraph(ctx)
    try:
        pg.set_limits(2000)
        for ml in (True, False):
            assert _separators(*long2, 0 if ml else 2) > PG.MAX_SEPARATORS
            out, status, chi2 = pg.optimise(batch, multilevel=ml, iters=(2, 1, 2))
            assert (status == PG.OK).all()
            for k, g in enumerate(batch):
                solo = (default if len(g[0]) < 200 else pg).optimise([g], multilevel=ml, iters=(2, 1, 2))   # the small ones: a default solver, dense
                assert np.array_equal(out[k], solo[0][0]) and np.array_equal(chi2[k], solo[2][0]), (ml, k)
    finally:
        pg.close()
        default.close()


def test_failure_paths(ctx):
    P, E = _long_graph()
    pg = PG.PoseGraph(ctx)
    try:
        for bad in ((0, 1), (-1, 1), (300, 0), (300, -5)):
            assert pg.L.rgbid_pg_set_limits(pg._h, *bad) == E_INVALID
            with pytest.raises(RgbidError):
                pg.set_limits(*bad)
        pg.set_limits(len(P))
        nan = E.copy()
        kf = np.flatnonzero(nan["type"] == PG.SEQ_KF)
        nan[kf[200]]["cov"][0] = np.nan
        for ml in (True, False):
            out, status, _ = pg.optimise([(P, nan), (P, E)], multilevel=ml)
            assert status.tolist() == [PG.NOT_PD, PG.OK]
            assert np.array_equal(out[0], P)
            assert np.array_equal(out[1], pg.optimise([(P, E)], multilevel=ml)[0][0])
        pg.set_limits(PG.MAX_SEPARATORS)                            # back to the default: refused again
        with pytest.raises(RgbidError):
            pg.optimise([(P, E)], multilevel=True)
    finally:
        pg.close()
