"""CPU tests of the pose-graph back-end: the SO(3) x R^3 maps, the analytic Jacobians against finite differences, the fixing and refusal
rules, the mirror's convergence, the C header and the library's exports.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from rgbid import _lib
from rgbid import posegraph as PG
from tests import pg_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("w", [0.3, 1e-7])   # the Rodrigues branch and the theta < 1e-5 branch (trafo_so3r3.h:229-240)
def test_log_exp_roundtrip(w):
    r = np.random.default_rng(1)
    for _ in range(20):
        d = np.concatenate([r.normal(0, 1, 3), r.normal(0, w, 3)])
        R, t = M.exp(d)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-12)
        assert np.allclose(M.log(R, t), d, rtol=1e-9, atol=1e-15)


def test_exp_small_branch_is_second_order():
    w = np.array([1e-6, -2e-6, 3e-6])
    R, _ = M.exp(np.concatenate([np.zeros(3), w]))
    S = M.skew(w)
    assert np.array_equal(R, np.eye(3) + S + 0.5 * S @ S)


def test_jacobians_match_finite_differences():
    """e(T_i (+) d) and e(T_j (+) d) by central differences against types_six_dof_pose.cpp:101-137 (Q^-1 R_E is the right-Jacobian
    inverse because jacobianR is the left Jacobian)"""
    r = np.random.default_rng(7)
    for _ in range(10):
        Ri, Rj, RZ = M.rand_rot(r, 0.5), M.rand_rot(r, 0.5), M.rand_rot(r, 0.5)
        ti, tj, tZ = r.normal(0, 1, 3), r.normal(0, 1, 3), r.normal(0, 1, 3)
        _, _, Ji, Jj = M.edge_terms(Ri, ti, Rj, tj, RZ, tZ, np.eye(6))
        h = 1e-6
        for which, J in (("i", Ji), ("j", Jj)):
            num = np.zeros((6, 6))
            for k in range(6):
                d = np.zeros(6)
                d[k] = h
                ep = []
                for s in (1, -1):
                    if which == "i":
                        Rp, tp = M.oplus(Ri, ti, s * d)
                        RE, tE = RZ @ Rj.T @ Rp, RZ @ Rj.T @ (tp - tj) + tZ
                    else:
                        Rp, tp = M.oplus(Rj, tj, s * d)
                        RE, tE = RZ @ Rp.T @ Ri, RZ @ Rp.T @ (ti - tp) + tZ
                    ep.append(M.log(RE, tE))
                num[:, k] = (ep[0] - ep[1]) / (2 * h)
            assert np.abs(num - J).max() <= 1e-6 * max(1.0, np.abs(J).max()), (which, np.abs(num - J).max())


def test_information_rederivation_at_zero_error():
    """at E = I, D = I: Omega is the constraint's information"""
    cov = np.diag([1e-4, 2e-4, 3e-4, 1e-5, 2e-5, 3e-5])
    _, Om, _, _ = M.edge_terms(np.eye(3), np.zeros(3), np.eye(3), np.zeros(3), np.eye(3), np.zeros(3), cov)
    assert np.allclose(Om, np.linalg.inv(cov), rtol=1e-12)


def _edges(rows):
    return PG.edges([(i, j, ty, np.eye(3), np.zeros(3), np.eye(6)) for i, j, ty in rows])


def test_fixing_rules():
    E = _edges([(0, 1, PG.SEQ_ODO), (1, 2, PG.SEQ_ODO), (5, 2, PG.LC_KF), (4, 7, PG.LC_KF)])
    f = PG.fixed_vertices(8, E)
    assert f.tolist() == [True, False, True, False, False, False, False, False]   # vertex 0 and min LC endpoint = 2
    assert M.fixed_vertices(8, E).tolist() == f.tolist()
    assert PG.fixed_vertices(3, _edges([(0, 1, PG.SEQ_KF)])).tolist() == [True, False, False]


def test_unanchored_components_are_refused():
    # level 2: keyframes 0-3 anchored through vertex 0; level 1 chain anchored through the keyframes
    ok = _edges([(0, 1, 0), (1, 2, 0), (2, 3, 0), (0, 3, PG.SEQ_KF)])
    assert PG.multilevel_anchored(4, ok)
    M.optimise(M.make_graph(np.random.default_rng(0), 4, K=2, L=0)[0], ok)   # solvable
    # a second chunk's keyframe chain 5 -> 8 touches no fixed vertex: multilevel refused, single level fine
    two = _edges([(k, k + 1, 0) for k in range(9)] + [(0, 3, PG.SEQ_KF), (5, 8, PG.SEQ_KF)])
    assert not PG.multilevel_anchored(10, two)
    P = np.tile(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), (10, 1))
    with pytest.raises(ValueError):
        M.optimise(P, two, multilevel=True)
    M.optimise(P, two, multilevel=False)
    assert PG.choose_mode([(P, two)]) == "single" and PG.choose_mode([(P[:4], ok)]) == "multilevel"
    # a seam-crossing loop anchors the second chain: its smallest endpoint is fixed
    loop = np.concatenate([two, _edges([(8, 3, PG.LC_KF)])])
    assert PG.multilevel_anchored(10, loop)


def test_mirror_reduces_error():
    r = np.random.default_rng(3)
    for ml in (True, False):
        P, E, GT = M.make_graph(r, 60, K=8, L=3, lost=(17,), drift=0.01, noise=1e-4)
        out = M.optimise(P, E, multilevel=ml)
        assert M.chi2(out, E) < 1e-3 * M.chi2(P, E)
        err0 = np.linalg.norm(P[:, 9:] - GT[:, 9:], axis=1).max()
        err1 = np.linalg.norm(out[:, 9:] - GT[:, 9:], axis=1).max()
        assert err1 < 0.5 * err0, (ml, err0, err1)


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_pg.c"
    src.write_text('#include "rgbid_posegraph.h"\n'
                   "typedef char edge_is_400_bytes[sizeof(rgbid_pg_edge) == 400 ? 1 : -1];\n"
                   "typedef char graph_is_16_bytes[sizeof(rgbid_pg_graph) == 16 ? 1 : -1];\n"
                   "int use(rgbid_pg* p) { int st[1]; double chi[2]; int it[3] = {10, 5, 10};\n"
                   "  return rgbid_pg_optimise(p, 0, 0, 0, 0, 1, it, st, chi) + RGBID_PG_LC_KF + RGBID_PG_MAX_SEPARATORS; }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_edge_dtype_matches_header():
    assert PG.EDGE_DTYPE.itemsize == 400 and PG.GRAPH_DTYPE.itemsize == 16
    assert PG.EDGE_DTYPE.fields["R"][1] == 16 and PG.EDGE_DTYPE.fields["t"][1] == 88 and PG.EDGE_DTYPE.fields["cov"][1] == 112


def test_library_exports_posegraph_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_posegraph.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_pg_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(PG.EXPORTS), set(declared) ^ set(PG.EXPORTS)
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def _rec(n, lost=(), first_status=1):
    from rgbid.dist import GATHER_DTYPE
    r = np.zeros(n, GATHER_DTYPE)
    for j in range(n):
        r[j]["frame_id"] = j
        r[j]["R"] = np.eye(3)
        r[j]["t"] = [0.01 * j, 0.0, 0.0]
        r[j]["cov"] = 100 * np.eye(6) if j in lost else (np.zeros((6, 6)) if j == 0 else 1e-4 * (1 + j) * np.eye(6))
        if j in lost:
            r[j]["t"] = 0.0
    return r


def test_graph_from_run_id_mapping():
    """two chunks sharing frame 4 (ranges (0, 4), (4, 9)): SEQ_ODO for records 1.. of each chunk, no edge for a chunk's record 0, chunk-local
    header ids shifted by the chunk's first frame, lost frames as recorded"""
    recs = [_rec(5, lost=(2,)), _rec(6)]
    F = 10
    R = np.tile(np.eye(3), (F, 1, 1)); t = np.arange(F * 3, dtype=float).reshape(F, 3)
    hdr = lambda i, j: dict(id=i, end_id=j, R_rel=np.eye(3), t_rel=np.array([i, j, 0.0]), cov_rel=np.eye(6) * (i + j + 1))
    P, E = PG.graph_from_run(R, t, recs, [0, 4], [(0, hdr(0, 3)), (1, hdr(0, 2)), (1, hdr(2, 5))])
    assert P.shape == (F, 12) and np.array_equal(P[:, 9:], t) and np.array_equal(P[:, :9], R.reshape(F, 9))
    odo = E[E["type"] == PG.SEQ_ODO]
    assert [(int(a), int(b)) for a, b in zip(odo["from"], odo["to"])] == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (8, 9)]
    assert np.array_equal(odo[1]["cov"].reshape(6, 6), 100 * np.eye(6)) and np.array_equal(odo[1]["t"], np.zeros(3))     # lost frame 2
    assert np.array_equal(odo[4]["cov"].reshape(6, 6), recs[1][1]["cov"]) and np.array_equal(odo[4]["t"], recs[1][1]["t"])  # chunk 1, record 1
    kf = E[E["type"] == PG.SEQ_KF]
    assert [(int(a), int(b)) for a, b in zip(kf["from"], kf["to"])] == [(0, 3), (4, 6), (6, 9)]
    assert np.array_equal(kf[2]["t"], [2, 5, 0]) and np.array_equal(kf[2]["cov"].reshape(6, 6), 8 * np.eye(6))
    # chunk 1's keyframe chain (4 -> 6 -> 9) touches no fixed vertex: multilevel unsolvable, "auto" picks single level
    assert PG.choose_mode([(P, E)]) == "single"
    # a seam-crossing loop anchors it
    lc = PG.edges([(9, 0, PG.LC_KF, np.eye(3), np.zeros(3), np.eye(6))])
    assert PG.choose_mode([(P, np.concatenate([E, lc]))]) == "multilevel"     # 4 -> 6 -> 9 -> 0 reaches the fixed vertex 0


def test_grey_kat():
    """cv::cvtColor(BGR2GRAY) fixed point on PixelRGB{r, g, b} bytes: byte 0 has the blue weight 1868"""
    c = np.array([[255, 255, 255], [0, 0, 0], [10, 20, 30], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 1, 1], [128, 64, 32]], np.uint8)
    expect = [255, 0, 22, 29, 150, 76, 1, (128 * 1868 + 64 * 9617 + 32 * 4899 + 8192) >> 14]
    assert PG.grey_from_colors(c).tolist() == expect
    assert expect[-1] == 62


def test_loop_proposal():
    """candidates: >= 3 exports apart, within radius and angle; per query the 2 most separated + the 2 nearest"""
    F = 12
    R = np.tile(np.eye(3), (F, 1, 1))
    t = np.zeros((F, 3))
    t[:, 0] = [0.0, 1.0, 2.0, 3.0, 0.05, 0.1, 0.2, 5.0, 0.01, 0.3, 0.02, 0.04]
    frames = list(range(F))
    out = PG.propose_loops(frames, R, t, radius=0.5, angle=0.5)
    by = {}
    for q, c in out:
        by.setdefault(q, []).append(c)
    assert by[4] == [0] and by[5] == [0] and by[6] == [0]
    assert by[11] == [0, 4, 5, 8]       # most separated 0, 4; nearest 8 (0.03), 5 (0.06) (10 is too close in export order)
    assert all(q - c >= 3 for q, c in out)
    R2 = R.copy()
    R2[11] = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]])   # 90 degrees away: no candidate for 11
    assert 11 not in {q for q, _ in PG.propose_loops(frames, R2, t, radius=0.5, angle=0.5)}
