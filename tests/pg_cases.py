"""The graphs the pose-graph solver (csrc/kernels_posegraph.hip) is held to the float64 mirror on: one small hand-built graph per structure that
selects a path of the host planner (pg_plan / build_stage) or of a kernel.  Plain numpy, no GPU.  Nothing here comes from
rgbid.posegraph.synthetic_graph.

A case is name -> (poses [V, 12], edges, expectation).  The poses are a drifted chain: the truth steps 1 cm and turns 0.01 rad per vertex, the
start is composed from steps that are off by 1 mm / 2 mrad each.  Every measurement is the truth's relative pose with 1e-4 noise, every covariance
1e-4 I, so each case is well conditioned and inside Gauss-Newton's basin (tests/test_cpu_posegraph_cases.py holds the table to that).

The expectation is written by hand, per stage (STAGES: multilevel level 2, multilevel level 1, the single level):
  sep     the separator vertices, ascending
  first   first(i) per separator: the first block column of row i of the reduced system's envelope
  seg     the segments (v0, m, has_A, has_B): a maximal run of free non-separator vertices v0 .. v0 + m - 1; has_A / has_B: v0 - 1 / v0 + m is free
  edges   the number of active edges
The rules (build_stage): vertex 0 and the smallest LC_KF endpoint are fixed; level 2 takes SEQ_KF / LC_KF, level 1 SEQ_ODO with every vertex
level 2 touched fixed, the single level everything.  A vertex is active when an active edge touches it, free when active and not fixed, a
separator when free with an active edge to anything but v - 1 / v + 1.

Edges are written (from, to, type); `o` = SEQ_ODO, `k` = SEQ_KF, `l` = LC_KF.  What each case is for:
  chain_kf               the baseline: keyframes 0, 3, 6 over an odometry chain.  Segment 4..5 lies between separators 3 and 6, which also share
                         the direct edge k(3, 6): S_AB and a separator-separator edge on one block
  neighbour_rev          chain_kf with every odometry edge stored from > to: PgInc::side swaps in pg_couple for G (towards A), C inside the run and
                         C towards B
  sse_rev                chain_kf with the keyframe edges stored from > to: PgSse a > b, the envelope's flag 0 instead of 2
  adjacent_separators    separators 2 and 3 are frame neighbours: their odometry edge is a separator-separator edge; _rev stores it from > to
  double_neighbour       k(2, 3) and k(3, 4) beside o(2, 3) and o(3, 4): two active edges on a frame-neighbour pair of different types make no
                         separator; pg_couple sums both for G (pair 2, 3) and for C inside the run (pair 3, 4).  _mixed stores the keyframe
                         edges from > to, so one sum takes a side-0 and a side-1 term
  double_sse             k(2, 5) and k(5, 2): two active edges between the same two separators, one in each direction
  mid_fixed              l(6, 3) fixes vertex 3 in the middle: segment 4..4 has no left separator although v0 > 0; _rev stores l(3, 6)
  inactive_gap           vertex 3 is in no edge: segment 4..4 has no left separator because v0 - 1 is inactive, segment 1..2 no right one
  tail_segment           one separator (ns = 1) and a segment 3..4 that runs to the end of the graph: no right separator
  sab_only               separators 2 and 4 tied to the fixed vertex 0 only: the segment 3..3 (length 1) between them is their only coupling
  lost_frame             no edge between 2 and 3 inside the run 1..5: C = 0 inside a segment
  lost_after_separator   no edge between separator 3 and the segment 4..5 it bounds: slotA is set and G = 0
  no_separators          keyframe edges between frame neighbours only: no separator in any stage (neither solver gets the graph)
  envelope_mixed_first   level 2: first = [0, 0, 2, 1, 2]; row 3 holds k = 2 with first(k) > first(3), row 4 holds k = 3 with first(k) < first(4)
  loop_row               l(10, 2) between the last and the first separator (l(4, 0) keeps vertex 0 the smallest LC_KF endpoint): the last
                         row's envelope spans the whole matrix; _rev stores l(2, 10)
  ns7, ns8, ns42, ns43   a keyframe every second vertex and k(2, 2 ns): ns * 36 and 6 * ns on either side of the reduced workgroup's 256 threads
  edges256, edges257     four odometry edges per pair and 4 / 5 keyframe edges: 256 / 257 active edges in the single level (k_pg_chi2_sum's stride)

BATCHES are lists of tiny graphs whose single-level totals of active edges, free vertices and segments come to 64 and to 65 (PG_T, the block of
the per-item kernels); at 65 the last graph's items lie on both sides of item 64.
"""
import functools
import zlib

import numpy as np

from rgbid import posegraph as PG
from tests import pg_mirror as M

SEED = 20261020
STAGES = ("level2", "level1", "single")       # rgbid_pg_envelope's stage 0, 1, 2
PG_T, PG_RT = 64, 256
ITERS = ((1, 0, 1), (2, 1, 2))
COV = 1e-4 * np.eye(6)
o, k, l = PG.SEQ_ODO, PG.SEQ_KF, PG.LC_KF
F, T = False, True


def build(name, V, spec):
    """-> (poses [V, 12], edges) of the graph with the edges spec = [(from, to, type), ...]"""
    rr = np.random.default_rng([SEED, zlib.crc32(name.encode())])
    Rg, tg = [np.eye(3)], [np.zeros(3)]
    Rs, ts = [np.eye(3)], [np.zeros(3)]
    for _ in range(1, V):
        dR, dt = M.rand_rot(rr, 0.01), np.array([0.01, 0.0, 0.0]) + rr.normal(0, 0.002, 3)
        tg.append(tg[-1] + Rg[-1] @ dt)
        Rg.append(Rg[-1] @ dR)
        dR, dt = dR @ M.rand_rot(rr, 2e-3), dt + rr.normal(0, 1e-3, 3)
        ts.append(ts[-1] + Rs[-1] @ dt)
        Rs.append(Rs[-1] @ dR)
    rows = []
    for a, b, ty in spec:   # E = Z Tb^-1 Ta = I at the truth: Z = Ta^-1 Tb
        rows.append((a, b, ty, Rg[a].T @ Rg[b] @ M.rand_rot(rr, 1e-4), Rg[a].T @ (tg[b] - tg[a]) + rr.normal(0, 1e-4, 3), COV))
    P = PG.poses_array(np.array(Rs), np.array(ts))
    P.setflags(write=False)
    E = PG.edges(rows)
    E.setflags(write=False)
    return P, E


def chain(V, skip=()):
    return [(v, v + 1, o) for v in range(V - 1) if v not in skip]


def rev(spec):
    return [(b, a, ty) for a, b, ty in spec]


def X(sep=(), first=(), seg=(), edges=0):
    return dict(sep=list(sep), first=list(first), seg=list(seg), edges=edges)


def _ns_case(ns):
    """keyframes 0, 2, .., 2 ns over an odometry chain, and k(2, 2 ns): the last row reaches back to the first"""
    V = 2 * ns + 1
    spec = chain(V) + [(2 * q - 2, 2 * q, k) for q in range(1, ns + 1)] + [(2, 2 * ns, k)]
    sep = list(range(2, 2 * ns + 1, 2))
    first = [0] + list(range(ns - 2)) + [0]
    return V, spec, dict(level2=X(sep, first, [], ns + 1),
                         level1=X(seg=[(2 * q - 1, 1, F, F) for q in range(1, ns + 1)], edges=2 * ns),
                         single=X(sep, first, [(1, 1, F, T)] + [(2 * q - 1, 1, T, T) for q in range(2, ns + 1)], 3 * ns + 1))


def _edges_case(nk):
    """64 vertices, four odometry edges per pair (252), keyframes 0, 2, .., 2 nk"""
    V = 64
    spec = [e for v in range(V - 1) for e in [(v, v + 1, o)] * 4] + [(2 * q - 2, 2 * q, k) for q in range(1, nk + 1)]
    sep = list(range(2, 2 * nk + 1, 2))
    first = [0] + list(range(nk - 1))
    tail = 2 * nk + 1
    return V, spec, dict(level2=X(sep, first, [], nk),
                         level1=X(seg=[(2 * q - 1, 1, F, F) for q in range(1, nk + 1)] + [(tail, V - tail, F, F)], edges=252),
                         single=X(sep, first, [(1, 1, F, T)] + [(2 * q - 1, 1, T, T) for q in range(2, nk + 1)] + [(tail, V - tail, T, F)], 252 + nk))


_CHAIN_KF = dict(level2=X([3, 6], [0, 0], [], 2),
                 level1=X(seg=[(1, 2, F, F), (4, 2, F, F)], edges=6),
                 single=X([3, 6], [0, 0], [(1, 2, F, T), (4, 2, T, T)], 8))
_ADJACENT = dict(level2=X([2, 3], [0, 1], [], 2),
                 level1=X(seg=[(1, 1, F, F), (4, 1, F, F)], edges=4),
                 single=X([2, 3], [0, 0], [(1, 1, F, T), (4, 1, T, F)], 6))
_DOUBLE_NEIGHBOUR = dict(level2=X([2], [0], [(3, 2, T, F)], 3),
                         level1=X(seg=[(1, 1, F, F), (5, 1, F, F)], edges=5),
                         single=X([2], [0], [(1, 1, F, T), (3, 3, T, F)], 8))
_MID_FIXED = dict(level2=X([2, 5, 6], [0, 0, 2], [], 3),
                  level1=X(seg=[(1, 1, F, F), (4, 1, F, F), (7, 1, F, F)], edges=7),
                  single=X([2, 5, 6], [0, 0, 1], [(1, 1, F, T), (4, 1, F, T), (7, 1, T, F)], 10))
_LOOP_ROW = dict(level2=X([2, 4, 6, 8, 10], [0, 0, 1, 2, 0], [], 7),
                 level1=X(seg=[(v, 1, F, F) for v in (1, 3, 5, 7, 9)], edges=10),
                 single=X([2, 4, 6, 8, 10], [0, 0, 1, 2, 0], [(1, 1, F, T)] + [(v, 1, T, T) for v in (3, 5, 7, 9)], 17))
_KF5 = [(0, 2, k), (2, 4, k), (4, 6, k), (6, 8, k), (8, 10, k)]

_SPECS = {
    "chain_kf": (7, chain(7) + [(0, 3, k), (3, 6, k)], _CHAIN_KF),
    "neighbour_rev": (7, rev(chain(7)) + [(0, 3, k), (3, 6, k)], _CHAIN_KF),
    "sse_rev": (7, chain(7) + [(3, 0, k), (6, 3, k)], _CHAIN_KF),
    "adjacent_separators": (5, chain(5) + [(0, 2, k), (0, 3, k)], _ADJACENT),
    "adjacent_separators_rev": (5, [(0, 1, o), (1, 2, o), (3, 2, o), (3, 4, o), (0, 2, k), (0, 3, k)], _ADJACENT),
    "double_neighbour": (6, chain(6) + [(0, 2, k), (2, 3, k), (3, 4, k)], _DOUBLE_NEIGHBOUR),
    "double_neighbour_mixed": (6, chain(6) + [(0, 2, k), (3, 2, k), (4, 3, k)], _DOUBLE_NEIGHBOUR),
    "double_sse": (6, chain(6) + [(0, 2, k), (2, 5, k), (5, 2, k)],
                   dict(level2=X([2, 5], [0, 0], [], 3),
                        level1=X(seg=[(1, 1, F, F), (3, 2, F, F)], edges=5),
                        single=X([2, 5], [0, 0], [(1, 1, F, T), (3, 2, T, T)], 8))),
    "mid_fixed": (8, chain(8) + [(0, 2, k), (2, 5, k), (6, 3, l)], _MID_FIXED),
    "mid_fixed_rev": (8, chain(8) + [(0, 2, k), (2, 5, k), (3, 6, l)], _MID_FIXED),
    "inactive_gap": (7, [(0, 1, o), (1, 2, o), (4, 5, o), (5, 6, o), (0, 5, k)],
                     dict(level2=X([5], [0], [], 1),
                          level1=X(seg=[(1, 2, F, F), (4, 1, F, F), (6, 1, F, F)], edges=4),
                          single=X([5], [0], [(1, 2, F, F), (4, 1, F, T), (6, 1, T, F)], 5))),
    "tail_segment": (5, chain(5) + [(0, 2, k)],
                     dict(level2=X([2], [0], [], 1),
                          level1=X(seg=[(1, 1, F, F), (3, 2, F, F)], edges=4),
                          single=X([2], [0], [(1, 1, F, T), (3, 2, T, F)], 5))),
    "sab_only": (5, chain(5) + [(0, 2, k), (0, 4, k)],
                 dict(level2=X([2, 4], [0, 1], [], 2),
                      level1=X(seg=[(1, 1, F, F), (3, 1, F, F)], edges=4),
                      single=X([2, 4], [0, 0], [(1, 1, F, T), (3, 1, T, T)], 6))),
    "lost_frame": (7, chain(7, skip=(2,)) + [(0, 6, k)],
                   dict(level2=X([6], [0], [], 1),
                        level1=X(seg=[(1, 5, F, F)], edges=5),
                        single=X([6], [0], [(1, 5, F, T)], 6))),
    "lost_after_separator": (7, chain(7, skip=(3,)) + [(0, 3, k), (3, 6, k)],
                             dict(level2=X([3, 6], [0, 0], [], 2),
                                  level1=X(seg=[(1, 2, F, F), (4, 2, F, F)], edges=5),
                                  single=X([3, 6], [0, 0], [(1, 2, F, T), (4, 2, T, T)], 7))),
    "no_separators": (4, chain(4) + [(0, 1, k), (1, 2, k)],
                      dict(level2=X(seg=[(1, 2, F, F)], edges=2),
                           level1=X(seg=[(3, 1, F, F)], edges=3),
                           single=X(seg=[(1, 3, F, F)], edges=5))),
    "envelope_mixed_first": (11, chain(11) + [(0, 2, k), (2, 4, k), (0, 6, k), (4, 8, k), (6, 10, k)],
                             dict(level2=X([2, 4, 6, 8, 10], [0, 0, 2, 1, 2], [], 5),
                                  level1=X(seg=[(v, 1, F, F) for v in (1, 3, 5, 7, 9)], edges=10),
                                  single=X([2, 4, 6, 8, 10], [0, 0, 1, 1, 2], [(1, 1, F, T)] + [(v, 1, T, T) for v in (3, 5, 7, 9)], 15))),
    "loop_row": (11, chain(11) + _KF5 + [(4, 0, l), (10, 2, l)], _LOOP_ROW),
    "loop_row_rev": (11, chain(11) + _KF5 + [(4, 0, l), (2, 10, l)], _LOOP_ROW),
    "ns7": _ns_case(7),
    "ns8": _ns_case(8),
    "ns42": _ns_case(42),
    "ns43": _ns_case(43),
    "edges256": _edges_case(4),
    "edges257": _edges_case(5),
}

CASES = {name: build(name, V, spec) + (expect,) for name, (V, spec, expect) in _SPECS.items()}

# the failure paths run on chain_kf: o(1, 2) lies inside segment 1..2, k(3, 6) joins the two separators
FAILURE_CASE, FAILURE_NEIGHBOUR = "chain_kf", "mid_fixed"
FAIL_ODO_EDGE, FAIL_SSE_EDGE = 1, 7


def with_nan(E, edge):
    """a copy of the edges with a NaN in the covariance of one"""
    E = E.copy()
    E[edge]["cov"][0] = np.nan
    return E


# ---- batches at the block size of the per-item kernels ----
# single-level items per tiny graph:                       edges  free  segments
_G2 = (2, [(0, 1, o), (0, 1, k)])                         #   2     1     1
_G4 = (4, chain(4) + [(0, 2, k)])                         #   4     3     2
_G5 = (5, chain(5) + [(0, 2, k)])                         #   5     4     2
_G6 = (6, chain(6) + [(0, 2, k)])                         #   6     5     2
_G6K = (6, chain(6) + [(0, 2, k), (2, 4, k)])             #   7     5     3


def _batch(name, members):
    return [build(f"{name}/{q}", V, spec) for q, (V, spec) in enumerate(members)]


# name -> (graphs, what is counted in the single-level stage, its total, the last graph's first item)
BATCHES = {
    "edges64": (_batch("edges64", [_G4] * 16), "edges", 64, 60),
    "edges65": (_batch("edges65", [_G4] * 15 + [_G5]), "edges", 65, 60),
    "free64": (_batch("free64", [_G4] * 21 + [_G2]), "free", 64, 63),
    "free65": (_batch("free65", [_G4] * 20 + [_G6]), "free", 65, 60),
    "segments64": (_batch("segments64", [_G4] * 32), "segments", 64, 62),
    "segments65": (_batch("segments65", [_G4] * 31 + [_G6K]), "segments", 65, 62),
}


@functools.lru_cache(maxsize=None)
def mirror(name, multilevel, iters):
    """the mirror's poses of a case (or of member q of a batch, name = "batch/q"), computed once and read-only"""
    if "/" in name:
        b, q = name.split("/")
        P, E = BATCHES[b][0][int(q)]
    else:
        P, E, _ = CASES[name]
    out = M.optimise(P, E, multilevel=multilevel, iters=iters)
    out.setflags(write=False)
    return out
