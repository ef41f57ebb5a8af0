"""GPU tests of the pose-graph solver on the hand-built graphs of tests/pg_cases.py: one graph per structure that selects a path of the host
planner or of a kernel, each held to the float64 mirror (tests/pg_mirror.py) after 1 and 2 Gauss-Newton steps per stage, where an error in one
branch has not yet been absorbed by convergence.  tests/test_cpu_posegraph_cases.py holds the table itself to the planner and to its own claims."""
import numpy as np
import pytest

from rgbid import posegraph as PG
from tests import pg_cases as C
from tests import pg_mirror as M

pytestmark = pytest.mark.gpu

CONFIGS = [(ml, it) for ml in (True, False) for it in C.ITERS]
BOUND = 1e-9       # m and rad: the bound of test_truncated_schedules_match_mirror


def _run(pg, graphs, ml, iters):
    out, status, chi2 = pg.optimise([g[:2] for g in graphs], multilevel=ml, iters=iters)
    return [(out[q], int(status[q]), chi2[q].copy()) for q in range(len(graphs))]


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2], equal_nan=True)


@pytest.fixture(scope="module")
def solo(ctx):
    """(case, multilevel, iters) -> (poses, status, chi2) of a default solver (dense reduced system) given that graph alone"""
    pg = PG.PoseGraph(ctx)
    try:
        return {(name, ml, it): _run(pg, [g], ml, it)[0] for name, g in C.CASES.items() for ml, it in CONFIGS}
    finally:
        pg.close()


@pytest.mark.parametrize("multilevel,iters", CONFIGS)
def test_cases_match_mirror(solo, multilevel, iters):
    """every case within 1e-9 m / 1e-9 rad of the mirror, chi2 before to rel 1e-9.
    Measured on an MI355X, worst case of the table (m / rad): (1, 0, 1) multilevel 3.3e-16 / 6.0e-16 (ns42) and single level 1.1e-15 / 2.4e-15
    (edges256), (2, 1, 2) multilevel 5.3e-16 / 1.9e-15 (edges256) and single level 1.1e-16 / 4.3e-17 (edges257); every case below ns42 within
    2.8e-17 / 1.1e-17 after (2, 1, 2), single level."""
    worst, bad = (0.0, 0.0, None), []
    for name, (P, E, _) in C.CASES.items():
        got, status, chi2 = solo[(name, multilevel, iters)]
        dt, ang = M.pose_err(got, C.mirror(name, multilevel, iters))
        E0 = E[E["type"] != PG.SEQ_ODO] if multilevel else E
        ref_chi = M.chi2(P, E0)
        print(f"{name}: {dt:.3e} m, {ang:.3e} rad, chi2 {chi2[0]:.9e} (mirror {ref_chi:.9e})")
        if max(dt, ang) >= max(worst[:2]):
            worst = (dt, ang, name)
        if status != PG.OK or not (dt <= BOUND and ang <= BOUND) or chi2[0] != pytest.approx(ref_chi, rel=1e-9):
            bad.append((name, status, dt, ang, chi2[0], ref_chi))
    print(f"iters {iters} {'multilevel' if multilevel else 'single level'}: max deviation {worst[0]:.3e} m, {worst[1]:.3e} rad ({worst[2]})")
    assert not bad, bad


def test_envelope_equals_dense_bytewise(ctx, solo):
    """set_limits(MAX_SEPARATORS, 1) hands every stage with a separator to the envelope solver: the bytes of the dense solver, for poses, status
    and chi2, on every case"""
    env = PG.PoseGraph(ctx)
    try:
        env.set_limits(PG.MAX_SEPARATORS, 1)
        bad = [(name, ml, it) for name, g in C.CASES.items() for ml, it in CONFIGS if not _same(_run(env, [g], ml, it)[0], solo[(name, ml, it)])]
    finally:
        env.close()
    assert not bad, bad


@pytest.mark.parametrize("envelope", [False, True])
def test_batch_equals_solo(ctx, solo, envelope):
    """all cases in one call, in table order and reversed: each result is the bytes of its solo run"""
    names = list(C.CASES)
    pg = PG.PoseGraph(ctx)
    try:
        if envelope:
            pg.set_limits(PG.MAX_SEPARATORS, 1)
        bad = []
        for order in (names, names[::-1]):
            for ml, it in CONFIGS:
                res = _run(pg, [C.CASES[n] for n in order], ml, it)
                bad += [(n, ml, it, order is names) for n, r in zip(order, res) if r[1] != PG.OK or not _same(r, solo[(n, ml, it)])]
    finally:
        pg.close()
    assert not bad, bad


@pytest.mark.parametrize("name", C.BATCHES)
def test_block_boundary_batches(ctx, name):
    """64 and 65 active edges / free vertices / segments in one call (PG_T = 64 threads per block of the per-item kernels): every member is the
    bytes of its solo run, and within 1e-9 of the mirror after (2, 1, 2).
    Measured on an MI355X, worst member of any batch: 7.8e-18 m / 1.3e-17 rad (free65)."""
    graphs = C.BATCHES[name][0]
    pg = PG.PoseGraph(ctx)
    try:
        bad, worst = [], (0.0, 0.0)
        for ml, it in CONFIGS:
            res = _run(pg, graphs, ml, it)
            for q, (g, r) in enumerate(zip(graphs, res)):
                if r[1] != PG.OK or not _same(r, _run(pg, [g], ml, it)[0]):
                    bad.append((q, ml, it, "solo"))
                if it == (2, 1, 2):
                    dt, ang = M.pose_err(r[0], C.mirror(f"{name}/{q}", ml, it))
                    worst = (max(worst[0], dt), max(worst[1], ang))
                    if not (dt <= BOUND and ang <= BOUND):
                        bad.append((q, ml, it, dt, ang))
    finally:
        pg.close()
    print(f"{name}: max deviation from the mirror {worst[0]:.3e} m, {worst[1]:.3e} rad")
    assert not bad, bad


def _failure_inputs():
    P, E, _ = C.CASES[C.FAILURE_CASE]
    return P, E, C.CASES[C.FAILURE_NEIGHBOUR]


def _fail(pg, P, E, edge, other, ml, it):
    """the clean pair first, on the same solver: its workspace then holds that call's updates, so a launch that did not skip the failed graph
    would move it (a fresh workspace may hold zeros, and a zero update leaves the poses as they are) -> (failed graph, its neighbour)"""
    clean = _run(pg, [(P, E), other], ml, it)
    assert [r[1] for r in clean] == [PG.OK, PG.OK] and not np.array_equal(clean[0][0], P)
    return _run(pg, [(P, C.with_nan(E, edge)), other], ml, it)


def test_failure_in_the_second_stage_keeps_the_first(ctx, solo):
    """a NaN covariance on an odometry edge, multilevel: level 2 does not see the edge and moves the poses, level 1's first segment pivot fails.
    The graph ends NOT_PD at the poses level 2 left, not at its input"""
    P, E, other = _failure_inputs()
    it = (2, 1, 2)
    pg = PG.PoseGraph(ctx)
    try:
        bad, ok = _fail(pg, P, E, C.FAIL_ODO_EDGE, other, True, it)
        stage_one = _run(pg, [(P, E)], True, (it[0], 0, 0))[0]
    finally:
        pg.close()
    assert (bad[1], ok[1], stage_one[1]) == (PG.NOT_PD, PG.OK, PG.OK)
    assert not np.array_equal(stage_one[0], P) and not np.array_equal(stage_one[0], solo[(C.FAILURE_CASE, True, it)][0])
    assert np.array_equal(bad[0], stage_one[0])
    assert _same(ok, solo[(C.FAILURE_NEIGHBOUR, True, it)])


def test_failure_raised_by_the_segment_kernel(ctx, solo):
    """the same NaN edge, single level: it lies inside a segment, whose first pivot fails in k_pg_segment; the poses are the input"""
    P, E, other = _failure_inputs()
    pg = PG.PoseGraph(ctx)
    try:
        bad, ok = _fail(pg, P, E, C.FAIL_ODO_EDGE, other, False, (2, 1, 2))
    finally:
        pg.close()
    assert (bad[1], ok[1]) == (PG.NOT_PD, PG.OK)
    assert np.array_equal(bad[0], P)
    assert _same(ok, solo[(C.FAILURE_NEIGHBOUR, False, (2, 1, 2))])


@pytest.mark.parametrize("envelope", [False, True])
@pytest.mark.parametrize("multilevel", [True, False])
def test_failure_raised_by_the_reduced_factorisation(ctx, solo, envelope, multilevel):
    """a NaN covariance on the edge between the two separators: every segment pivot is finite, the reduced system's first pivot is not.  NOT_PD
    from the dense and from the envelope factorisation, the poses are the input"""
    P, E, other = _failure_inputs()
    pg = PG.PoseGraph(ctx)
    try:
        if envelope:
            pg.set_limits(PG.MAX_SEPARATORS, 1)
        bad, ok = _fail(pg, P, E, C.FAIL_SSE_EDGE, other, multilevel, (2, 1, 2))
    finally:
        pg.close()
    assert (bad[1], ok[1]) == (PG.NOT_PD, PG.OK)
    assert np.array_equal(bad[0], P)
    assert _same(ok, solo[(C.FAILURE_NEIGHBOUR, multilevel, (2, 1, 2))])
