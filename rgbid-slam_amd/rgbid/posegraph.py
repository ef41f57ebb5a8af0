"""Batched pose-graph optimisation on the device (binding of include/rgbid_posegraph.h): the reference's PoseGraph
(src/pose_graph_manager.cpp:76-245), g2o's SO(3) x R^3 Gauss-Newton, for many graphs in one call.

A graph is (poses [V, 12] = R row-major | t, edges: structured array of EDGE_DTYPE with graph-local vertex ids).  `PoseGraph.optimise`
runs the multilevel schedule (10 iterations over SEQ_KF / LC_KF, then 5 over SEQ_ODO with the keyframes fixed) or the single-level one
(10 over all edges) and returns the optimised poses, a status per graph and chi2 before / after.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ci, vp

SEQ_ODO, SEQ_KF, LC_KF = 0, 1, 2
OK, NOT_PD = 0, 1
MAX_SEPARATORS = 256
DEFAULT_ITERS = (10, 5, 10)

EDGE_DTYPE = np.dtype([("from", "<i4"), ("to", "<i4"), ("type", "<i4"), ("reserved", "<i4"), ("R", "<f8", (9,)), ("t", "<f8", (3,)),
                       ("cov", "<f8", (36,))])
assert EDGE_DTYPE.itemsize == 400
GRAPH_DTYPE = np.dtype([("v0", "<i4"), ("n_vertices", "<i4"), ("e0", "<i4"), ("n_edges", "<i4")])

SIGNATURES = {
    "rgbid_pg_create": (vp, vp),
    "rgbid_pg_destroy": (vp,),
    "rgbid_pg_optimise": (vp, ci, vp, vp, vp, ci, vp, vp, vp),
    "rgbid_pg_set_limits": (vp, ci, ci),
    "rgbid_pg_envelope": (ci, ci, vp, ci, ci, vp, vp, vp),
    "rgbid_pg_set_timing": (vp, ci),
    "rgbid_pg_last_times": (vp, vp, vp),
    "rgbid_pg_last_work": (vp, vp, vp, vp),
}
EXPORTS = list(SIGNATURES)


def edges(rows):
    """[(from, to, type, R (3x3), t (3), cov (6x6)), ...] -> structured array of EDGE_DTYPE"""
    out = np.zeros(len(rows), EDGE_DTYPE)
    for k, (i, j, ty, R, t, cov) in enumerate(rows):
        out[k]["from"], out[k]["to"], out[k]["type"] = int(i), int(j), int(ty)
        out[k]["R"] = np.asarray(R, np.float64).reshape(9)
        out[k]["t"] = np.asarray(t, np.float64).reshape(3)
        out[k]["cov"] = np.asarray(cov, np.float64).reshape(36)
    return out


def poses_array(R, t):
    """R [V, 3, 3], t [V, 3] -> [V, 12]"""
    R = np.asarray(R, np.float64).reshape(-1, 9)
    return np.ascontiguousarray(np.concatenate([R, np.asarray(t, np.float64).reshape(-1, 3)], 1))


def _components_anchored(nv, e, fixed):
    par = list(range(nv))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x
    act = np.zeros(nv, bool)
    for a, b in zip(e["from"], e["to"]):
        par[find(int(a))] = find(int(b))
        act[a] = act[b] = True
    anch = {find(v) for v in range(nv) if act[v] and fixed[v]}
    return all(find(v) in anch for v in range(nv) if act[v])


def fixed_vertices(nv, e):
    """the vertices buildGraph fixes (pose_graph_manager.cpp:89-151): vertex 0 and the smallest LC_KF endpoint"""
    fixed = np.zeros(nv, bool)
    fixed[0] = True
    lc = e[e["type"] == LC_KF]
    if len(lc):
        fixed[int(min(lc["from"].min(), lc["to"].min()))] = True
    return fixed


def multilevel_anchored(nv, e):
    """True when every component of the level-2 edges (SEQ_KF, LC_KF) holds a fixed vertex, so that the multilevel schedule is solvable"""
    return _components_anchored(nv, e[e["type"] != SEQ_ODO], fixed_vertices(nv, e))


def choose_mode(graphs):
    """optimise="auto": multilevel when every graph's level-2 components are anchored, else single level"""
    return "multilevel" if all(multilevel_anchored(len(p), e) for p, e in graphs) else "single"


class PoseGraph(_lib.CtxHandle):
    """Device pose-graph solver on a context's device and stream."""

    _destroy, _signatures = "rgbid_pg_destroy", SIGNATURES

    def __init__(self, ctx):
        super().__init__(ctx)
        self._created(self.L.rgbid_pg_create(C.byref(self._h), ctx._h))

    def set_timing(self, on):
        check(self.L.rgbid_pg_set_timing(self._h, int(bool(on))))

    def set_limits(self, max_separators, envelope_from=None):
        """max_separators: graphs with more separators in a stage are refused (default MAX_SEPARATORS).  envelope_from: stages with at least
        this many separators go to the envelope factorisation instead of the dense one (None = the default MAX_SEPARATORS + 1: exactly the
        graphs the dense solver cannot take; 1 = always).  The results do not depend on envelope_from."""
        check(self.L.rgbid_pg_set_limits(self._h, int(max_separators), MAX_SEPARATORS + 1 if envelope_from is None else int(envelope_from)))

    def last_times(self):
        """(ms [linearise, assemble, segment, reduced, backsub + update, chi2, whole call on the device], launches) of the last timed call"""
        ms = (C.c_double * 7)()
        n = C.c_int()
        check(self.L.rgbid_pg_last_times(self._h, ms, C.byref(n)))
        return np.array(ms[:]), n.value

    def last_work(self):
        """(reduced-system flops, linearise bytes, segment bytes) of the last call"""
        v = [C.c_double() for _ in range(3)]
        check(self.L.rgbid_pg_last_work(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def optimise_flat(self, ranges, poses, edges, multilevel=True, iters=None):
        """ranges: GRAPH_DTYPE array; poses [V, 12] float64 (copied); edges EDGE_DTYPE array -> (poses, status, chi2 [G, 2])"""
        ranges = np.ascontiguousarray(ranges, GRAPH_DTYPE)
        P = np.ascontiguousarray(poses, np.float64).copy()
        E = np.ascontiguousarray(edges, EDGE_DTYPE)
        G = len(ranges)
        status = np.zeros(max(G, 1), np.int32)
        chi2 = np.zeros((max(G, 1), 2), np.float64)
        it = None if iters is None else (C.c_int * 3)(*[int(x) for x in iters])
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(self.L.rgbid_pg_optimise(self._h, G, p(ranges), p(P), p(E) if len(E) else None, int(bool(multilevel)), it, p(status), p(chi2)))
        return P, status[:G], chi2[:G]

    def optimise(self, graphs, multilevel=True, iters=None):
        """graphs: [(poses [V, 12], edges EDGE_DTYPE), ...] -> ([poses [V, 12]], status [G], chi2 [G, 2])"""
        ranges = np.zeros(len(graphs), GRAPH_DTYPE)
        v = e = 0
        for g, (P, E) in enumerate(graphs):
            ranges[g] = (v, len(P), e, len(E))
            v += len(P)
            e += len(E)
        P = np.concatenate([np.asarray(P, np.float64).reshape(-1, 12) for P, _ in graphs]) if graphs else np.zeros((0, 12))
        E = np.concatenate([np.asarray(E, EDGE_DTYPE) for _, E in graphs]) if graphs else np.zeros(0, EDGE_DTYPE)
        out, status, chi2 = self.optimise_flat(ranges, P, E, multilevel, iters)
        return [out[r["v0"]:r["v0"] + r["n_vertices"]] for r in ranges], status, chi2


def envelope(n_vertices, edges, stage):
    """Host only: the separators of a stage (0 / 1: multilevel level 2 / level 1, 2: single level) of one graph and the block envelope of its
    reduced system -> (sep_vertex [ns], first [ns]): first[i] is the first block column of block row i."""
    L = _lib.bind(SIGNATURES)
    E = np.ascontiguousarray(edges, EDGE_DTYPE)
    n = C.c_int()
    sv = np.zeros(max(int(n_vertices), 1), np.int32)
    fi = np.zeros(max(int(n_vertices), 1), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    check(L.rgbid_pg_envelope(int(n_vertices), len(E), p(E) if len(E) else None, int(stage), len(sv), C.byref(n), p(sv), p(fi)))
    return sv[:n.value].copy(), fi[:n.value].copy()


# ---- graphs from a run of the engine ----
def _rot_angle(R):
    return float(np.arccos(np.clip((np.trace(R) - 1) / 2, -1.0, 1.0)))


def grey_from_colors(colors):
    """Keyframe::grey_image_ as processNewKeyframe forms it (keyframe_manager.cpp:307): cv::cvtColor(BGR2GRAY) on the PixelRGB{r, g, b} bytes,
    so byte 0 gets the BLUE weight.  OpenCV's fixed-point form: (b0 * 1868 + b1 * 9617 + b2 * 4899 + 8192) >> 14 (its published
    coefficients 0.114 / 0.587 / 0.299 scaled by 2^14; OpenCV is not available to this project, so this is not checked against it)."""
    c = np.asarray(colors, np.uint8).astype(np.int32)
    return ((c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def graph_from_run(R, t, chunk_records, first_frames, headers=()):
    """One graph of a sequence from what a (chunked) run produced.

    R [F, 3, 3], t [F, 3]: the composed trajectory (the initial poses).  chunk_records[c]: the gathered records (rgbid.dist.GATHER_DTYPE) of
    chunk c, one per frame of the chunk; first_frames[c]: the chunk's first global frame.  headers: [(chunk, keyframe header dict with id,
    end_id, R_rel, t_rel, cov_rel)] of the exports (Engine.read_keyframe).
    Record j >= 1 of chunk c gives SEQ_ODO (f0 + j - 1 -> f0 + j) with its dT and covariance (lost frames already carry identity and 100 I,
    visodo.cpp:2066-2078); a chunk's record 0 gives no edge: its frame is the previous chunk's last frame, one vertex.  A header gives
    SEQ_KF (f0 + id -> f0 + end_id) with R_rel | t_rel and cov_rel (visodo.cpp:1646).  -> (poses [F, 12], edges EDGE_DTYPE)"""
    rows = []
    for rec, f0 in zip(chunk_records, first_frames):
        for j in range(1, len(rec)):
            rows.append((f0 + j - 1, f0 + j, SEQ_ODO, rec[j]["R"], rec[j]["t"], rec[j]["cov"]))
    for c, h in headers:
        f0 = first_frames[c]
        rows.append((f0 + int(h["id"]), f0 + int(h["end_id"]), SEQ_KF, h["R_rel"], h["t_rel"], h["cov_rel"]))
    return poses_array(R, t), edges(rows)


def _relative(R, t, a, b):
    """T_a^-1 T_b: the measurement of an edge a -> b at the trajectory R, t"""
    return R[a].T @ R[b], R[a].T @ (t[b] - t[a])


def propose_loops(frames, R, t, radius=0.5, angle=0.5, min_separation=3, per_query=(2, 2)):
    """The project's stand-in for appearance-based detection (loop_closer.cpp:241-283 picks candidates by BoW score; that needs ORB + DBoW2):
    for each exported keyframe q (in export order) the earlier exports c with q - c >= min_separation (MIN_KF_SEPARATION = 3,
    config_data/visodoRGBDconfig.ini) whose camera centre is within `radius` m and whose relative rotation is within `angle` rad at the
    trajectory R, t; of those, the per_query[0] with the largest separation and the per_query[1] nearest.  frames: global frame of each export.
    -> [(q, c)] export indices"""
    out = []
    for q in range(len(frames)):
        cands = []
        for c in range(q - min_separation + 1):
            d = float(np.linalg.norm(t[frames[q]] - t[frames[c]]))
            if d <= radius and _rot_angle(R[frames[q]].T @ R[frames[c]]) <= angle:
                cands.append((c, d))
        if not cands:
            continue
        pick = [c for c, _ in sorted(cands, key=lambda x: x[0])[:per_query[0]]]
        for c, _ in sorted(cands, key=lambda x: (x[1], x[0])):
            if len(pick) >= per_query[0] + per_query[1]:
                break
            if c not in pick:
                pick.append(c)
        out += [(q, c) for c in sorted(pick)]
    return out


def loop_constraints(ctx, keyframes, R, t, K, pairs=None, radius=0.5, angle=0.5, gate=(0.1, 0.1), min_separation=3, batch=64, guess=None):
    """LC_KF constraints from the dense verifier (KfAlign.align, KeyframeAlign::alignKeyframes) over candidate pairs of exported keyframes.

    keyframes: [dict(frame=global frame, depthinv=float32 [rows, cols], colors=uint8 [rows, cols, 3])] in export order; R, t: the current
    trajectory (the initial guess of each pair is its relative pose there -- the reference starts from RANSAC's, which needs ORB features);
    pairs: [(query, candidate)] export indices, or None = propose_loops(radius, angle, min_separation).  Every result becomes LC_KF(query,
    candidate, R, t, cov) as at loop_closer.cpp:319-325 when R, t and cov are finite, cov is positive definite and the correction to the
    guess is below gate = (metres, radians).  -> (edges EDGE_DTYPE with global frame ids, [dict(query, candidate, accepted, correction)])"""
    from .kfalign import KfAlign
    frames = [int(k["frame"]) for k in keyframes]
    if pairs is None:
        pairs = propose_loops(frames, R, t, radius, angle, min_separation)
    pairs = [(int(q), int(c)) for q, c in pairs]
    if guess is not None and len(guess) != len(pairs):
        raise ValueError(f"guess: one (R, t) per pair, got {len(guess)} for {len(pairs)} pairs")
    given = guess
    rows, report = [], []
    if not pairs:
        return edges(rows), report
    h, w = keyframes[0]["depthinv"].shape
    grey = [grey_from_colors(k["colors"]) for k in keyframes]
    al = KfAlign(ctx, h, w, min(batch, len(pairs)))
    try:
        for s in range(0, len(pairs), batch):
            chunk = pairs[s:s + batch]
            if given is None:
                guess = [_relative(R, t, frames[q], frames[c]) for q, c in chunk]
            else:
                guess = [(np.asarray(g[0], np.float64).reshape(3, 3), np.asarray(g[1], np.float64).reshape(3)) for g in given[s:s + batch]]
            Ra, ta, cov = al.align(np.stack([keyframes[q]["depthinv"] for q, _ in chunk]), np.stack([grey[q] for q, _ in chunk]),
                                   np.stack([keyframes[c]["depthinv"] for _, c in chunk]), np.stack([grey[c] for _, c in chunk]), K,
                                   np.stack([g[0] for g in guess]), np.stack([g[1] for g in guess]))
            for k, (q, c) in enumerate(chunk):
                R0, t0 = guess[k]
                ok = bool(np.isfinite(Ra[k]).all() and np.isfinite(ta[k]).all() and np.isfinite(cov[k]).all())
                corr = (float("inf"), float("inf"))
                if ok:
                    corr = (float(np.linalg.norm(R0.T @ (ta[k] - t0))), _rot_angle(R0.T @ Ra[k]))
                    try:
                        np.linalg.cholesky(0.5 * (cov[k] + cov[k].T))
                    except np.linalg.LinAlgError:
                        ok = False
                    ok = ok and corr[0] <= gate[0] and corr[1] <= gate[1]
                if ok:
                    rows.append((frames[q], frames[c], LC_KF, Ra[k], ta[k], cov[k]))
                report.append(dict(query=q, candidate=c, accepted=ok, correction=corr, **({} if given is None else dict(R=Ra[k].copy(), t=ta[k].copy(), guess=guess[k]))))
    finally:
        al.close()
    return edges(rows), report


def optimise_run(ctx, R, t, chunk_records, first_frames, headers, keyframes, K, optimise="auto", loops=None, **loop_kw):
    """graph_from_run + loop_constraints + one device optimisation: -> (R [F, 3, 3], t [F, 3], info dict(mode, status, chi2, loops)).
    loops: None, "auto" (candidates by distance on the trajectory), "appearance" (rgbid.loopfeat.appearance_loops: features, appearance
    proposal and RANSAC, no pose involved; each report row of a verified pair then also holds score, matches, inliers and hull ratios, and
    info["appearance"] lists every proposed pair; levels=, scale= among the keywords choose its feature pyramid, one level by default;
    proposal="bow", vocabulary=, shortlist_size= shortlist the candidates with a binary vocabulary, rgbid.bow; mask_level=, segment_k=,
    segment_min= keep the features of a negentropy mask, rgbid.segment: the keyframes then also hold overlap_mask and normals) or a list
    of (kf_a, kf_b)."""
    if optimise not in ("auto", "multilevel", "single"):
        raise ValueError(f"optimise must be 'auto', 'multilevel' or 'single', not {optimise!r}")
    P, E = graph_from_run(R, t, chunk_records, first_frames, headers)
    report = []
    if loops is not None:
        if isinstance(loops, str) and loops not in ("auto", "appearance"):
            raise ValueError(f"loops must be None, 'auto', 'appearance' or a list of (kf_a, kf_b), not {loops!r}")
        if isinstance(loops, str) and loops == "appearance":
            from . import loopfeat
            akw = {k: loop_kw.pop(k) for k in ("max_keypoints", "score_threshold", "per_query", "levels", "scale", "proposal", "vocabulary", "shortlist_size", "mask_level",
                                               "segment_k", "segment_min", "mask_out", "max_segments", "blocks")
                   if k in loop_kw}
            pairs, guess, appearance = loopfeat.appearance_loops(ctx, keyframes, K, min_separation=loop_kw.get("min_separation", 3), **akw)
            lc, report = loop_constraints(ctx, keyframes, R, t, K, pairs, guess=guess, **loop_kw)
            by_pair = {(a["query"], a["candidate"]): a for a in appearance}
            for row in report:
                a = by_pair[(row["query"], row["candidate"])]
                row.update({k: a[k] for k in ("score", "matches", "inliers", "hull_query", "hull_candidate")})
        else:
            pairs = None if isinstance(loops, str) else list(loops)
            lc, report = loop_constraints(ctx, keyframes, R, t, K, pairs, **loop_kw)
        E = np.concatenate([E, lc])
    mode = choose_mode([(P, E)]) if optimise == "auto" else optimise
    appearance = appearance if isinstance(loops, str) and loops == "appearance" else None
    pg = PoseGraph(ctx)
    try:
        # a long run has more separators than the dense reduced solver takes: those stages go to the envelope solver (same bytes below the cap)
        pg.set_limits(max(MAX_SEPARATORS, len(P)))
        out, status, chi2 = pg.optimise([(P, E)], multilevel=mode == "multilevel")
    finally:
        pg.close()
    Ro = out[0][:, :9].reshape(-1, 3, 3).copy()
    to = out[0][:, 9:].copy()
    return Ro, to, dict(mode=mode, status=int(status[0]), chi2=chi2[0].copy(), loops=report,
                        accepted=sum(1 for r in report if r["accepted"]), edges=E, **({} if appearance is None else dict(appearance=appearance)))


# ---- synthetic graphs (tests, tools/posegraph_bench.py) ----
def _rand_rot(r, scale):
    """Rodrigues of a normal(0, scale) rotation vector (so3r3.h exp)"""
    w = r.normal(0, scale, 3)
    th = np.linalg.norm(w)
    S = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-5:
        return np.eye(3) + S + 0.5 * S @ S
    return np.eye(3) + np.sin(th) / th * S + (1 - np.cos(th)) / th ** 2 * (S @ S)


def synthetic_graph(r, T, K=6, L=2, lost=(), drift=0.01, noise=1e-3, loops_to_start=False):
    """a chain of T poses with SEQ_ODO edges (lost frames: identity, cov 100 I), SEQ_KF edges between K keyframes and L loop edges between
    keyframes at least 3 apart (loops_to_start: from later keyframes to keyframe 0, the fixed vertex); measurements are the ground truth perturbed by `noise`, initial poses composed from drifted odometry.
    -> (poses [T, 12], edges, ground truth [T, 12])"""
    Rg, tg = [np.eye(3)], [np.zeros(3)]
    for k in range(1, T):
        Rg.append(Rg[-1] @ _rand_rot(r, 0.02))
        tg.append(tg[-1] + Rg[-1] @ np.array([0.02, 0.0, 0.01]) + r.normal(0, 0.005, 3))

    def rel(i, j):   # Z with E = Z Tj^-1 Ti = I at the truth: Z = Ti^-1 Tj
        R = Rg[i].T @ Rg[j]
        t = Rg[i].T @ (tg[j] - tg[i])
        return R, t

    def noisy(R, t, s):
        return R @ _rand_rot(r, s), t + r.normal(0, s, 3)
    rows = []
    for k in range(1, T):
        if k in lost:
            rows.append((k - 1, k, SEQ_ODO, np.eye(3), np.zeros(3), 100 * np.eye(6)))
        else:
            R, t = noisy(*rel(k - 1, k), noise)
            c = np.diag(r.uniform(0.5, 2.0, 6)) * 1e-4
            rows.append((k - 1, k, SEQ_ODO, R, t, c))
    kfs = sorted(set([0] + list(r.choice(np.arange(1, T), size=min(K - 1, T - 1), replace=False))))
    for a, b in zip(kfs[:-1], kfs[1:]):
        R, t = noisy(*rel(a, b), noise)
        rows.append((a, b, SEQ_KF, R, t, np.eye(6) * 1e-4))
    for _ in range(L):
        if len(kfs) < 5:
            break
        a = 0 if loops_to_start else int(r.integers(0, len(kfs) - 4))
        b = int(r.integers(a + 3, len(kfs)))
        R, t = noisy(*rel(kfs[b], kfs[a]), noise)
        rows.append((kfs[b], kfs[a], LC_KF, R, t, np.eye(6) * 1e-4))
    E = np.zeros(len(rows), EDGE_DTYPE)
    for k, (i, j, ty, R, t, c) in enumerate(rows):
        E[k]["from"], E[k]["to"], E[k]["type"] = i, j, ty
        E[k]["R"], E[k]["t"], E[k]["cov"] = R.reshape(9), t, np.asarray(c).reshape(36)
    # initial: odometry with drift
    P = np.zeros((T, 12))
    P[0, :9] = np.eye(3).reshape(9)
    for k in range(1, T):
        ed = E[k - 1]
        Z_R, Z_t = ed["R"].reshape(3, 3) @ _rand_rot(r, drift), ed["t"] + r.normal(0, drift, 3)
        Rp = P[k - 1, :9].reshape(3, 3)
        P[k, :9] = (Rp @ Z_R).reshape(9)
        P[k, 9:] = Rp @ Z_t + P[k - 1, 9:]
    GT = np.concatenate([np.array(Rg).reshape(T, 9), np.array(tg)], 1)
    return P, E, GT
