"""float64 numpy mirror of the pose-graph back-end (include/rgbid/so3r3.h, include/rgbid_posegraph.h): g2o's SO(3) x R^3 vertex and
edge (ThirdParty/g2o-lite/g2o/types/pose_graph/), the fixing rules and schedules of PoseGraph (src/pose_graph_manager.cpp:76-209), and
Gauss-Newton with a dense np.linalg.solve over the free vertices.  The device solver must agree with it to tolerance."""
import numpy as np

SEQ_ODO, SEQ_KF, LC_KF = 0, 1, 2


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def deltaR(R):
    return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


def jacobianR(w):
    S = skew(w)
    th = np.linalg.norm(w)
    if th < 1e-5:
        return np.eye(3) + 0.5 * S + S @ S / 6.0
    return np.eye(3) + (1 - np.cos(th)) / th ** 2 * S + (1 - np.sin(th) / th) / th ** 2 * (S @ S)


def exp(d):
    """(upsilon, omega) -> (R, t = upsilon)"""
    d = np.asarray(d, np.float64)
    w = d[3:]
    th = np.linalg.norm(w)
    S = skew(w)
    if th < 1e-5:
        R = np.eye(3) + S + 0.5 * S @ S
    else:
        R = np.eye(3) + np.sin(th) / th * S + (1 - np.cos(th)) / th ** 2 * (S @ S)
    return R, d[:3].copy()


def log(R, t):
    d = 0.5 * (np.trace(R) - 1)
    dR = deltaR(R)
    s = 0.5 if d > 0.99999 else np.arccos(d) / (2 * np.sqrt(1 - d * d))
    return np.concatenate([np.asarray(t, np.float64), s * dR])


def oplus(R, t, d):
    Rd, td = exp(d)
    return R @ Rd, R @ td + t


def edge_terms(Ri, ti, Rj, tj, RZ, tZ, cov):
    """-> e, Omega, Ji, Jj (types_six_dof_pose.h:84-104, types_six_dof_pose.cpp:101-137)"""
    RE = RZ @ (Rj.T @ Ri)
    mtji = Rj.T @ (ti - tj)
    tE = RZ @ mtji + tZ
    e = log(RE, tE)
    Qinv = np.linalg.inv(jacobianR(e[3:]))
    D = np.zeros((6, 6))
    D[:3, :3] = np.eye(3)
    D[:3, 3:] = -skew(tE)
    D[3:, 3:] = Qinv @ RE.T
    proto_inv = np.linalg.inv(np.linalg.inv(cov))
    Om = np.linalg.inv(D @ proto_inv @ D.T)
    Ji = np.zeros((6, 6))
    Ji[:3, :3] = RE
    Ji[3:, 3:] = Qinv @ RE
    Jj = np.zeros((6, 6))
    Jj[:3, :3] = -RZ
    Jj[:3, 3:] = RZ @ skew(mtji)
    Jj[3:, 3:] = -Qinv @ RZ
    return e, Om, Ji, Jj


def edge_error(P, ed):
    """e of one edge at poses P [V, 12]"""
    i, j = int(ed["from"]), int(ed["to"])
    Pi, Pj = P[i], P[j]
    RE = ed["R"].reshape(3, 3) @ (Pj[:9].reshape(3, 3).T @ Pi[:9].reshape(3, 3))
    tE = ed["R"].reshape(3, 3) @ (Pj[:9].reshape(3, 3).T @ (Pi[9:] - Pj[9:])) + ed["t"]
    return log(RE, tE)


def _terms(P, ed):
    i, j = int(ed["from"]), int(ed["to"])
    return edge_terms(P[i, :9].reshape(3, 3), P[i, 9:], P[j, :9].reshape(3, 3), P[j, 9:], ed["R"].reshape(3, 3), ed["t"], ed["cov"].reshape(6, 6))


def chi2(P, E):
    s = 0.0
    for ed in E:
        e, Om, _, _ = _terms(P, ed)
        s += float(e @ Om @ e)
    return s


def fixed_vertices(nv, E):
    fixed = np.zeros(nv, bool)
    fixed[0] = True
    lc = E[E["type"] == LC_KF]
    if len(lc):
        fixed[int(min(lc["from"].min(), lc["to"].min()))] = True
    return fixed


def check_anchored(nv, E, fixed):
    par = list(range(nv))

    def find(x):
        while par[x] != x:
            x = par[x]
        return x
    act = np.zeros(nv, bool)
    for ed in E:
        a, b = int(ed["from"]), int(ed["to"])
        par[find(a)] = find(b)
        act[a] = act[b] = True
    anch = {find(v) for v in range(nv) if act[v] and fixed[v]}
    if not all(find(v) in anch for v in range(nv) if act[v]):
        raise ValueError("a component of the active edges has no fixed vertex")


def gauss_newton(P, E, fixed, iters):
    """iters iterations over the edges E; updates P in place"""
    nv = len(P)
    act = np.zeros(nv, bool)
    for ed in E:
        act[int(ed["from"])] = act[int(ed["to"])] = True
    free = [v for v in range(nv) if act[v] and not fixed[v]]
    idx = {v: k for k, v in enumerate(free)}
    n = 6 * len(free)
    if n == 0:
        return
    for _ in range(iters):
        H = np.zeros((n, n))
        b = np.zeros(n)
        for ed in E:
            e, Om, Ji, Jj = _terms(P, ed)
            blocks = [(idx.get(int(ed["from"])), Ji), (idx.get(int(ed["to"])), Jj)]
            for a, Ja in blocks:
                if a is None:
                    continue
                b[6 * a:6 * a + 6] -= Ja.T @ Om @ e
                for c, Jc in blocks:
                    if c is not None:
                        H[6 * a:6 * a + 6, 6 * c:6 * c + 6] += Ja.T @ Om @ Jc
        dx = np.linalg.solve(H, b)
        for v, k in idx.items():
            R, t = oplus(P[v, :9].reshape(3, 3), P[v, 9:], dx[6 * k:6 * k + 6])
            P[v, :9] = R.reshape(9)
            P[v, 9:] = t


def optimise(P, E, multilevel=True, iters=(10, 5, 10)):
    """one graph: poses [V, 12], edges (EDGE_DTYPE) -> optimised poses (a copy)"""
    P = np.array(P, np.float64, copy=True)
    fixed = fixed_vertices(len(P), E)
    if multilevel:
        E2 = E[E["type"] != SEQ_ODO]
        E1 = E[E["type"] == SEQ_ODO]
        check_anchored(len(P), E2, fixed)
        f1 = fixed.copy()
        for ed in E2:
            f1[int(ed["from"])] = f1[int(ed["to"])] = True
        check_anchored(len(P), E1, f1)
        gauss_newton(P, E2, fixed, iters[0])
        gauss_newton(P, E1, f1, iters[1])
    else:
        check_anchored(len(P), E, fixed)
        gauss_newton(P, E, fixed, iters[2])
    return P


def stages(P, E):
    """(stage id of rgbid_pg_envelope, active edges, fixed flags) of multilevel level 2, multilevel level 1 and the single level"""
    fixed = fixed_vertices(len(P), E)
    E2, E1 = E[E["type"] != SEQ_ODO], E[E["type"] == SEQ_ODO]
    f1 = fixed.copy()
    for ed in E2:
        f1[int(ed["from"])] = f1[int(ed["to"])] = True
    return [(0, E2, fixed), (1, E1, f1), (2, E, fixed)]


def hessian(P, E, fixed):
    """H over the free active vertices (gauss_newton's assembly) -> (H, free vertices)"""
    nv = len(P)
    act = np.zeros(nv, bool)
    for ed in E:
        act[int(ed["from"])] = act[int(ed["to"])] = True
    free = [v for v in range(nv) if act[v] and not fixed[v]]
    idx = {v: k for k, v in enumerate(free)}
    H = np.zeros((6 * len(free), 6 * len(free)))
    for ed in E:
        _, Om, Ji, Jj = _terms(P, ed)
        blocks = [(idx.get(int(ed["from"])), Ji), (idx.get(int(ed["to"])), Jj)]
        for a, Ja in blocks:
            for c, Jc in blocks:
                if a is not None and c is not None:
                    H[6 * a:6 * a + 6, 6 * c:6 * c + 6] += Ja.T @ Om @ Jc
    return H, free


def pose_err(a, b):
    """max translation difference (m) and max rotation angle (rad) between two pose sets [V, 12]"""
    dt = np.abs(a[:, 9:] - b[:, 9:]).max()
    ang = 0.0
    for x, y in zip(a, b):   # |deltaR(Ra^T Rb)| / 2 = sin(angle): exact at small angles, where arccos of the trace is not
        ang = max(ang, float(np.linalg.norm(deltaR(x[:9].reshape(3, 3).T @ y[:9].reshape(3, 3)))) / 2)
    return dt, ang


# ---- synthetic graphs ----
def rand_rot(r, scale):
    return exp(np.concatenate([np.zeros(3), r.normal(0, scale, 3)]))[0]


def comb(ns):
    """vertex 0 (fixed) and separators 2, 4, .., 2 ns, each tied to vertex 0 and to the separator before it"""
    from rgbid import posegraph as PG
    n = 2 * ns + 2
    rr = np.random.default_rng(ns)
    rows = [(0, k, SEQ_KF, rand_rot(rr, 0.01), rr.normal(0, 0.01, 3), np.eye(6) * 1e-4) for k in range(2, 2 * ns + 1, 2)]
    rows += [(k - 2, k, SEQ_KF, rand_rot(rr, 0.01), rr.normal(0, 0.01, 3), np.eye(6) * 1e-4) for k in range(4, 2 * ns + 1, 2)]
    return np.tile(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), (n, 1)), PG.edges(rows)


def make_graph(r, T, K=6, L=2, lost=(), drift=0.01, noise=1e-3, loops_to_start=False):
    """rgbid.posegraph.synthetic_graph (the generator lives in the package so that tools can use it)"""
    from rgbid.posegraph import synthetic_graph
    return synthetic_graph(r, T, K, L, lost, drift, noise, loops_to_start)
