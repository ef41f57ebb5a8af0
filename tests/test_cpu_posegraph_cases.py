"""What keeps tests/test_gpu_posegraph_cases.py honest (no GPU): the table of tests/pg_cases.py is what it says it is.

  - the host planner (rgbid_pg_envelope: pg_plan / build_stage without a device) finds the separators and first(i) the table wrote down by hand,
    for every case and stage; the segments and the active edges, which the binding does not expose, are held to a restatement of the rule (_plan)
  - the float64 mirror solves every case in both schedules and moves the poses, and its H is well conditioned: the 1e-9 the device is held to
    then measures the device.  A condition on the inputs, checked on the reference alone
  - the table reaches every structure it was built for (test_the_table_reaches_every_structure), so a case cannot silently leave it
"""
import numpy as np
import pytest

from rgbid import posegraph as PG
from tests import pg_cases as C
from tests import pg_mirror as M

# cond(H) * 2^-52 * |dx| bounds the relative error a backward-stable float64 solve of H dx = b can show.  The steps of these graphs are below
# 0.1 (m, rad), so under this cap two correct solvers agree to 1e6 * 2.2e-16 * 0.1 = 2.2e-11: a fiftieth of the 1e-9 the device is held to.
COND_CAP = 1e6


def _plan(nv, E, stage):
    """the rule of build_stage -> (separators, segments (v0, m, has_A, has_B), number of active edges, free vertices)"""
    _, A, fixed = M.stages(np.zeros((nv, 12)), E)[stage]
    act = {int(v) for ed in A for v in (ed["from"], ed["to"])}
    free = [v in act and not fixed[v] for v in range(nv)] + [False]
    sep = {int(v) for ed in A if abs(int(ed["from"]) - int(ed["to"])) != 1 for v in (ed["from"], ed["to"]) if free[v]}
    seg, v = [], 0
    while v < nv:
        w = v
        while free[w] and w not in sep:
            w += 1
        if w > v:
            seg.append((v, w - v, v > 0 and free[v - 1], free[w]))
        v = max(w, v + 1)
    return sorted(sep), seg, len(A), [v for v in range(nv) if free[v]]


@pytest.mark.parametrize("name", C.CASES)
def test_planner_matches_the_table(name):
    P, E, expect = C.CASES[name]
    assert 3 <= len(P) <= 100
    for stage, key in enumerate(C.STAGES):
        x = expect[key]
        sv, first = PG.envelope(len(P), E, stage)
        assert sv.tolist() == x["sep"], (name, key)
        assert first.tolist() == x["first"], (name, key)
        sep, seg, edges, _ = _plan(len(P), E, stage)
        assert sep == x["sep"] and seg == x["seg"] and edges == x["edges"], (name, key, sep, seg, edges)


_cond = {}


@pytest.mark.parametrize("name", C.CASES)
def test_mirror_solves_and_is_well_conditioned(name):
    """Largest cond(H) at a stage's first iteration, measured: 7.8e3 (edges256, single level: the run of 55 vertices past the last keyframe);
    level 2 at most 1.3e3 (ns43), level 1 at most 6.4e3 (edges256), every case below ns42 under 1.1e2.  The cap is 1e6."""
    P, E, _ = C.CASES[name]
    for ml in (True, False):
        for iters in C.ITERS:
            ref = C.mirror(name, ml, iters)
            assert np.isfinite(ref).all() and float(np.abs(ref - P).max()) > 1e-6, (name, ml, iters)
    after2 = M.optimise(P, E, multilevel=True, iters=(2, 0, 0))
    for (stage, A, fixed), key in zip(M.stages(P, E), C.STAGES):
        H, free = M.hessian(after2 if stage == 1 else P, A, fixed)    # level 1 starts from level 2's result
        assert len(free) > 0, (name, key)
        cond = float(np.linalg.cond(H))
        _cond[(name, key)] = cond
        assert cond < COND_CAP, (name, key, cond)
    print(f"{name}: cond(H) " + ", ".join(f"{key} {_cond[(name, key)]:.2e}" for key in C.STAGES))


def _stage_views():
    """(name, stage key, expectation, active edges as (from, to, type), segment of every segment vertex, fixed flags)"""
    for name, (P, E, expect) in C.CASES.items():
        for (stage, A, fixed), key in zip(M.stages(P, E), C.STAGES):
            x = expect[key]
            seg_of = {v: q for q, (v0, m, _, _) in enumerate(x["seg"]) for v in range(v0, v0 + m)}
            yield name, key, x, [(int(e["from"]), int(e["to"]), int(e["type"])) for e in A], seg_of, fixed


def test_the_table_reaches_every_structure():
    """from the hand-written expectations and the edges: each structure the table was built for is in it (the name of a reaching case and
    stage is kept, so a failure says which structure lost its case)"""
    hit = {}
    for name, key, x, A, seg_of, fixed in _stage_views():
        sep, first, seg = x["sep"], x["first"], x["seg"]
        sidx = {v: q for q, v in enumerate(sep)}
        act = {v for a, b, _ in A for v in (a, b)}
        pairs = {}
        for a, b, ty in A:
            pairs.setdefault((min(a, b), max(a, b)), []).append((a, b, ty))
        mark = lambda what: hit.setdefault(what, (name, key))
        for a, b, ty in A:
            d = "reversed" if a > b else "forward"
            if a in sidx and b in sidx:
                mark(f"{d} separator-separator edge")
                if abs(a - b) == 1:
                    mark(f"{d} separator-separator edge between frame neighbours")
            elif abs(a - b) == 1 and a in seg_of and b in seg_of:
                mark(f"{d} neighbour edge inside a segment")
            elif abs(a - b) == 1 and (a in seg_of or b in seg_of) and (a in sidx or b in sidx):
                s, v = (a, b) if a in sidx else (b, a)
                mark(f"{d} edge between a segment and its {'left' if s < v else 'right'} separator")
            elif fixed[min(a, b)] and min(a, b) > 0 and ty == PG.LC_KF:
                mark(f"{d} LC_KF edge to the vertex it fixes in the middle")
        for (a, b), es in pairs.items():
            if len(es) < 2:
                continue
            dirs = "both directions" if len({e[0] for e in es}) == 2 else "one direction"
            if a in sidx and b in sidx:
                mark(f"two edges between two separators, {dirs}")
            elif b - a == 1 and len({e[2] for e in es}) == 2 and not (a in sidx and b in sidx):
                where = "inside a segment" if a in seg_of and b in seg_of else "between a segment and its separator" if a in seg_of or b in seg_of else None
                if where:
                    mark(f"ODO + KF on a frame-neighbour pair {where}, {dirs}")
        for v0, m, hasA, hasB in seg:
            if not hasA and v0 > 1 and fixed[v0 - 1] and v0 - 1 in act and key == "single":   # v0 - 1 > 0: not the first pose
                mark("segment with no left separator at v0 > 0: the vertex before it is fixed")
            if not hasA and v0 > 0 and v0 - 1 not in act:
                mark("segment with no left separator at v0 > 0: the vertex before it is inactive")
            if not hasB and hasA:
                mark("segment with a left and no right separator")
            if m == 1 and hasA and hasB:
                mark("segment of length 1 between two separators")
            if m == 1 and not hasA and not hasB:
                mark("segment of length 1 with no separator")
            if hasA and hasB:
                mark("segment whose separators share a direct edge" if (v0 - 1, v0 + m) in pairs else "segment whose separators share no edge")
            if any((v, v + 1) not in pairs for v in range(v0, v0 + m - 1)):
                mark("lost frame inside a segment")
            if hasA and (v0 - 1, v0) not in pairs:
                mark("lost frame between a separator and its segment")
        if key == "single" and not sep and A:
            mark("single level without separators")
        if len(sep) == 1:
            mark("one separator")
        for i, fi in enumerate(first):
            for q in range(fi + 1, i):
                if first[q] > fi:
                    mark("first(k) > first(i) inside row i")
            for q in range(fi + 1, i):
                if first[q] < fi:
                    mark("first(k) < first(i) inside row i")
        if len(sep) >= 4 and first[-1] == 0:
            mark("loop row spanning the whole matrix")
            if any(a in sidx and b in sidx and {sidx[a], sidx[b]} == {0, len(sep) - 1} for a, b, _ in A):
                mark(f"loop row stored {'from > to' if any(a > b and a in sidx and b in sidx and sidx[b] == 0 and sidx[a] == len(sep) - 1 for a, b, _ in A) else 'from < to'}")
        for ns in (7, 8, 42, 43):
            if len(sep) == ns:
                mark(f"{ns} separators")
        for n in (C.PG_RT, C.PG_RT + 1):
            if len(A) == n:
                mark(f"{n} active edges")
    wanted = [f"{d} {w}" for d in ("forward", "reversed") for w in (
        "separator-separator edge", "separator-separator edge between frame neighbours", "neighbour edge inside a segment",
        "edge between a segment and its left separator", "edge between a segment and its right separator", "LC_KF edge to the vertex it fixes in the middle")]
    wanted += ["two edges between two separators, both directions",
               "ODO + KF on a frame-neighbour pair inside a segment, one direction", "ODO + KF on a frame-neighbour pair inside a segment, both directions",
               "ODO + KF on a frame-neighbour pair between a segment and its separator, one direction",
               "ODO + KF on a frame-neighbour pair between a segment and its separator, both directions",
               "segment with no left separator at v0 > 0: the vertex before it is fixed", "segment with no left separator at v0 > 0: the vertex before it is inactive",
               "segment with a left and no right separator", "segment of length 1 between two separators", "segment of length 1 with no separator",
               "segment whose separators share a direct edge", "segment whose separators share no edge", "lost frame inside a segment",
               "lost frame between a separator and its segment", "single level without separators", "one separator",
               "first(k) > first(i) inside row i", "first(k) < first(i) inside row i", "loop row spanning the whole matrix", "loop row stored from > to",
               "loop row stored from < to", "7 separators", "8 separators", "42 separators", "43 separators", "256 active edges", "257 active edges"]
    for w in wanted:
        print(f"{w}: {hit.get(w)}")
    missing = [w for w in wanted if w not in hit]
    assert not missing, missing
    # the thresholds those counts stand for (k_pg_reduced: PG_RT threads over ns * 36 diagonal entries and over 6 * ns rows)
    assert 7 * 36 < C.PG_RT < 8 * 36 and 6 * 42 < C.PG_RT < 6 * 43


@pytest.mark.parametrize("name", C.BATCHES)
def test_batches_sit_on_the_block_boundary(name):
    graphs, what, total, last_from = C.BATCHES[name]
    counts = []
    for P, E in graphs:
        _, seg, edges, free = _plan(len(P), E, 2)
        counts.append(dict(edges=edges, free=len(free), segments=len(seg))[what])
        assert PG.multilevel_anchored(len(P), E)
    assert sum(counts) == total and total in (C.PG_T, C.PG_T + 1)
    assert sum(counts[:-1]) == last_from
    if total == C.PG_T + 1:   # the last graph's items lie on both sides of the block boundary
        assert last_from < C.PG_T - 1 and counts[-1] >= 3
    for q in range(len(graphs)):
        for ml in (True, False):
            ref = C.mirror(f"{name}/{q}", ml, (2, 1, 2))
            assert float(np.abs(ref - graphs[q][0]).max()) > 1e-6


def test_failure_case_edges_are_where_the_tests_need_them():
    P, E, expect = C.CASES[C.FAILURE_CASE]
    x = expect["single"]
    a, b = int(E[C.FAIL_ODO_EDGE]["from"]), int(E[C.FAIL_ODO_EDGE]["to"])
    assert E[C.FAIL_ODO_EDGE]["type"] == PG.SEQ_ODO and any(v0 <= a < v0 + m and v0 <= b < v0 + m for v0, m, _, _ in x["seg"])
    a, b = int(E[C.FAIL_SSE_EDGE]["from"]), int(E[C.FAIL_SSE_EDGE]["to"])
    assert E[C.FAIL_SSE_EDGE]["type"] == PG.SEQ_KF and a in x["sep"] and b in x["sep"] and a in expect["level2"]["sep"] and b in expect["level2"]["sep"]
    # with the NaN on k(3, 6) every segment pivot of the single level is still finite: the failure is the reduced factorisation's to raise
    seg_vertices = {v for v0, m, _, _ in x["seg"] for v in range(v0, v0 + m)}
    assert a not in seg_vertices and b not in seg_vertices
    assert np.isnan(C.with_nan(E, C.FAIL_SSE_EDGE)[C.FAIL_SSE_EDGE]["cov"][0]) and np.isfinite(E["cov"]).all()
