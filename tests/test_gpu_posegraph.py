"""GPU tests of the batched pose-graph solver (include/rgbid_posegraph.h) against the float64 mirror (tests/pg_mirror.py)."""
import numpy as np
import pytest

from rgbid import posegraph as PG
from rgbid._lib import RgbidError
from tests import pg_mirror as M
from tests.pg_mirror import comb as _comb, pose_err as _pose_err

pytestmark = pytest.mark.gpu


def _batch(seed, n):
    r = np.random.default_rng(seed)
    graphs = []
    for g in range(n):
        T = int(r.integers(5, 120))
        lost = tuple(int(x) for x in r.integers(1, T, size=int(r.integers(0, 3))))
        graphs.append(M.make_graph(r, T, K=int(r.integers(2, 12)), L=int(r.integers(0, 4)), lost=lost, drift=0.005, noise=1e-4)[:2])
    return graphs


@pytest.mark.parametrize("multilevel", [True, False])
def test_random_batches_match_mirror(ctx, multilevel):
    graphs = _batch(11 + multilevel, 24)
    pg = PG.PoseGraph(ctx)
    try:
        out, status, chi2 = pg.optimise(graphs, multilevel=multilevel)
    finally:
        pg.close()
    assert (status == PG.OK).all()
    worst = (0.0, 0.0)
    for (P, E), got in zip(graphs, out):
        ref = M.optimise(P, E, multilevel=multilevel)
        dt, ang = _pose_err(got, ref)
        worst = (max(worst[0], dt), max(worst[1], ang))
    for g, (P, E) in enumerate(graphs):   # g2o's activeChi2: the first stage's edges before, the last stage's after
        E0, E1 = (E[E["type"] != PG.SEQ_ODO], E[E["type"] == PG.SEQ_ODO]) if multilevel else (E, E)
        assert chi2[g, 0] == pytest.approx(M.chi2(P, E0), rel=1e-9)
        assert chi2[g, 1] == pytest.approx(M.chi2(out[g], E1), rel=1e-6, abs=1e-9)
    print(f"max deviation from the mirror ({'multilevel' if multilevel else 'single level'}): {worst[0]:.3e} m, {worst[1]:.3e} rad")
    assert worst[0] <= 1e-7 and worst[1] <= 1e-7, worst


@pytest.mark.parametrize("iters", [(1, 0, 1), (2, 1, 2), (0, 3, 3)])
def test_truncated_schedules_match_mirror(ctx, iters):
    """after 1 or 2 non-converged Gauss-Newton steps per stage the device state equals the mirror's: a wrong iteration count, a stage
    skipped or run twice, or an error in one step would show here (the full schedule converges to the same fixed point regardless)"""
    graphs = _batch(31, 12)
    pg = PG.PoseGraph(ctx)
    try:
        for ml in (True, False):
            out, status, _ = pg.optimise(graphs, multilevel=ml, iters=iters)
            assert (status == PG.OK).all()
            worst = (0.0, 0.0)
            moved = 0.0
            for (P, E), got in zip(graphs, out):
                ref = M.optimise(P, E, multilevel=ml, iters=iters)
                dt, ang = _pose_err(got, ref)
                worst = (max(worst[0], dt), max(worst[1], ang))
                moved = max(moved, float(np.abs(ref - P).max()))
            print(f"iters {iters} {'multilevel' if ml else 'single level'}: max deviation {worst[0]:.3e} m, {worst[1]:.3e} rad")
            assert worst[0] <= 1e-9 and worst[1] <= 1e-9, (iters, ml, worst)
            assert moved > 1e-4                   # the steps did move the poses
    finally:
        pg.close()


def test_bitwise_reproducible_and_batch_independent(ctx):
    r = np.random.default_rng(5)
    target = M.make_graph(r, 150, K=12, L=4, lost=(40,), drift=0.01, noise=1e-4)[:2]
    small = [M.make_graph(r, int(r.integers(3, 12)), K=3, L=1)[:2] for _ in range(16)]
    batch = [small[k % 16] for k in range(2047)]
    batch.insert(1234, target)
    pg = PG.PoseGraph(ctx)
    try:
        for ml in (True, False):
            a, sa, ca = pg.optimise([target], multilevel=ml)
            b, sb, cb = pg.optimise([target], multilevel=ml)
            assert np.array_equal(a[0], b[0]) and np.array_equal(ca, cb)
            big, sbig, cbig = pg.optimise(batch, multilevel=ml)
            assert (sbig == PG.OK).all()
            assert np.array_equal(big[1234], a[0]), ml
            assert np.array_equal(cbig[1234], ca[0])
            assert np.array_equal(big[0], pg.optimise([small[0]], multilevel=ml)[0][0])
    finally:
        pg.close()


def test_loops_remove_drift(ctx):
    """drifted odometry with ground-truth-consistent loop edges: the optimised trajectory loses most of its error"""
    # the loops close on keyframe 0, the fixed vertex (the smallest LC_KF endpoint is fixed at its drifted pose otherwise).  Measured on this
    # graph: ATE 0.109 m -> 4.8e-5 m (multilevel) / 4.9e-5 m (single level), 4.5e-4 of it; the bound is 1e-2 of it
    r = np.random.default_rng(21)
    P, E, GT = M.make_graph(r, 300, K=25, L=8, drift=0.005, noise=1e-5, loops_to_start=True)
    pg = PG.PoseGraph(ctx)
    try:
        for ml in (True, False):
            out, status, chi2 = pg.optimise([(P, E)], multilevel=ml)
            ate = lambda X: float(np.sqrt(np.mean(np.sum((X[:, 9:] - GT[:, 9:]) ** 2, 1))))
            before, after = ate(P), ate(out[0])
            print(f"ATE ({'multilevel' if ml else 'single level'}) before {before:.4f} m, after {after:.3e} m ({after / before:.2e} of it); "
                  f"chi2 {chi2[0, 0]:.3e} -> {chi2[0, 1]:.3e}")
            assert status[0] == PG.OK
            assert after < 1e-2 * before
    finally:
        pg.close()


def test_refusals_and_numerical_failure(ctx):
    r = np.random.default_rng(2)
    P, E, _ = M.make_graph(r, 30, K=4, L=0)
    pg = PG.PoseGraph(ctx)
    try:
        # refused before any launch: the caller's poses are untouched (the raw C-ABI call writes into this very array)
        ranges = np.zeros(1, PG.GRAPH_DTYPE)
        for bad, ml in ((PG.edges([(20, 25, PG.SEQ_KF, np.eye(3), np.zeros(3), np.eye(6))]), True),      # unanchored level-2 component
                        (PG.edges([(3, 3, PG.SEQ_ODO, np.eye(3), np.zeros(3), np.eye(6))]), False)):    # self edge
            ranges[0] = (0, len(P), 0, len(bad))
            Pc = P.copy()
            st = np.full(1, 7, np.int32)
            chi = np.full((1, 2), 7.0)
            import ctypes as C
            ptr = lambda a: a.ctypes.data_as(C.c_void_p)
            err = pg.L.rgbid_pg_optimise(pg._h, 1, ptr(ranges), ptr(Pc), ptr(bad), int(ml), None, ptr(st), ptr(chi))
            assert err == -1 and np.array_equal(Pc, P) and st[0] == 7 and (chi == 7.0).all()
            with pytest.raises(RgbidError):
                pg.optimise([(P, bad)], multilevel=ml)
        # exactly RGBID_PG_MAX_SEPARATORS separators are solved (the reduced right-hand side fills its LDS vector), one more is refused
        for ns, ok in ((PG.MAX_SEPARATORS, True), (PG.MAX_SEPARATORS + 1, False)):
            Pm, many = _comb(ns)                # vertex 0 (fixed) and separators 2, 4, .., 2 ns
            if ok:
                out, status, _ = pg.optimise([(Pm, many)], multilevel=True, iters=(2, 0, 0))
                ref = M.optimise(Pm, many, multilevel=True, iters=(2, 0, 0))
                dt, ang = _pose_err(out[0], ref)
                print(f"{ns} separators: max deviation {dt:.3e} m, {ang:.3e} rad")
                assert status[0] == PG.OK and dt <= 1e-9 and ang <= 1e-9
            else:
                with pytest.raises(RgbidError):
                    pg.optimise([(Pm, many)], multilevel=True)
        # a NaN covariance: that graph stops with RGBID_PG_NOT_PD and keeps its input poses; its neighbour is unaffected
        nan = E.copy()
        nan[3]["cov"][0] = np.nan
        out, status, _ = pg.optimise([(P, nan), (P, E)], multilevel=False)
        assert status.tolist() == [PG.NOT_PD, PG.OK]
        assert np.array_equal(out[0], P)
        assert np.array_equal(out[1], pg.optimise([(P, E)], multilevel=False)[0][0])
    finally:
        pg.close()


def test_kfalign_accepts_every_pair_count(ctx):
    """KfAlign sized for 127 pairs accepts 65 .. 127 (the creation-time sizing sampled 1 .. 64 and powers of two only)"""
    from rgbid.kfalign import KfAlign
    rows, cols = 120, 160
    r = np.random.default_rng(0)
    a = KfAlign(ctx, rows, cols, 127)
    try:
        for n in (65, 97, 127):
            iD = r.uniform(0.3, 1.0, (n, rows, cols)).astype(np.float32)
            g = r.integers(0, 255, (n, rows, cols)).astype(np.uint8)
            R, t, cov = a.align(iD, g, iD, g, (131.25, 131.25, 79.875, 59.875))
            assert R.shape == (n, 3, 3)
    finally:
        a.close()
