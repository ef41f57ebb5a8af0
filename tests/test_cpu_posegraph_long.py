"""CPU tests of the envelope reduced-system solver's host side: the header, the exports, and the envelope layout (rgbid_pg_envelope)
against the float64 mirror's H.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from rgbid import _lib
from rgbid import posegraph as PG
from tests import pg_mirror as M
from tests.pg_mirror import hessian as _mirror_H, stages as _stages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_with_set_limits_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_pg_limits.c"
    src.write_text('#include "rgbid_posegraph.h"\n'
                   "typedef char cap_is_256[RGBID_PG_MAX_SEPARATORS == 256 ? 1 : -1];\n"
                   "int use(rgbid_pg* p, const rgbid_pg_edge* e) { int n; int32_t sv[4], first[4];\n"
                   "  return rgbid_pg_set_limits(p, 5000, RGBID_PG_MAX_SEPARATORS + 1) + rgbid_pg_envelope(4, 3, e, 2, 4, &n, sv, first); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_library_exports_set_limits():
    assert "rgbid_pg_set_limits" in PG.EXPORTS and "rgbid_pg_envelope" in PG.EXPORTS
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "rgbid_pg_set_limits") and hasattr(L, "rgbid_pg_envelope")
    assert PG.MAX_SEPARATORS == 256 and hasattr(PG.PoseGraph, "set_limits")


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_envelope_layout_matches_mirror_structure(seed):
    """first(i) is the first non-zero block of row i of the reduced matrix (the Schur complement of the mirror's H on the separators), and
    its block Cholesky factor has no non-zero outside the envelope"""
    r = np.random.default_rng(100 + seed)
    T = int(r.integers(40, 90))
    lost = (int(r.integers(1, T)),)
    P, E, _ = M.make_graph(r, T, K=int(r.integers(6, 16)), L=int(r.integers(0, 5)), lost=lost, drift=0.005, noise=1e-4)
    for stage, Ea, fixed in _stages(P, E):
        sv, first = PG.envelope(len(P), E, stage)
        H, free = _mirror_H(P, Ea, fixed)
        # separators as the header defines them: free vertices with an active edge to anything but a frame-order neighbour
        sep = sorted({int(v) for ed in Ea if abs(int(ed["from"]) - int(ed["to"])) != 1 for v in (ed["from"], ed["to"])} & set(free))
        assert sv.tolist() == sep, stage
        if not sep:
            continue
        pos = {v: k for k, v in enumerate(free)}
        s_idx = np.concatenate([np.arange(6 * pos[v], 6 * pos[v] + 6) for v in sep])
        o_idx = np.setdiff1d(np.arange(len(H)), s_idx)
        S = H[np.ix_(s_idx, s_idx)]
        if len(o_idx):
            S = S - H[np.ix_(s_idx, o_idx)] @ np.linalg.solve(H[np.ix_(o_idx, o_idx)], H[np.ix_(o_idx, s_idx)])
        ns = len(sep)
        scale = np.abs(S).max()
        nz = lambda A: np.array([[np.abs(A[6 * i:6 * i + 6, 6 * j:6 * j + 6]).max() > 1e-9 * scale for j in range(ns)] for i in range(ns)])
        Snz = nz(S)
        assert [int(np.flatnonzero(Snz[i])[0]) for i in range(ns)] == first.tolist(), stage
        assert (first <= np.arange(ns)).all()
        Lnz = nz(np.linalg.cholesky(0.5 * (S + S.T)))
        for i in range(ns):
            assert not Lnz[i, :first[i]].any(), (stage, i)


def test_envelope_refuses_what_optimise_refuses():
    bad = PG.edges([(3, 3, PG.SEQ_ODO, np.eye(3), np.zeros(3), np.eye(6))])
    with pytest.raises(_lib.RgbidError):
        PG.envelope(10, bad, 2)
    unanchored = PG.edges([(5, 8, PG.SEQ_KF, np.eye(3), np.zeros(3), np.eye(6))])
    with pytest.raises(_lib.RgbidError):
        PG.envelope(10, unanchored, 0)
