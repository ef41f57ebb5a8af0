"""Integer / float32 / float64 numpy restatement of the loop-feature contract (include/rgbid_loopfeat.h).  The GPU
tests compare the features and the matches with it byte for byte, and the RANSAC's choice (best iteration, inlier count, mask) exactly;
the RANSAC pose is computed here in two independent ways (SVD with determinant correction, Horn's quaternion), neither of which is the
device's closed form."""
import numpy as np

from rgbid import loopfeat as LF
from tests.test_cpu_cloud import kinv_numpy

f32, f64 = np.float32, np.float64
PI = 3.14159265358979323846


# ---- tables ----
def pattern():
    """the project's test pattern: xorshift32 from 0x9E3779B9; a coordinate is (next % 27) - 13; a test (x1, y1, x2, y2) is accepted when both
    points lie in the disc of radius 13 and differ; the first 256 accepted"""
    s = 0x9E3779B9
    out = []

    def nxt():
        nonlocal s
        s ^= (s << 13) & 0xFFFFFFFF
        s ^= s >> 17
        s ^= (s << 5) & 0xFFFFFFFF
        return s
    while len(out) < LF.TESTS:
        v = [nxt() % 27 - 13 for _ in range(4)]
        if v[0] ** 2 + v[1] ** 2 > 169 or v[2] ** 2 + v[3] ** 2 > 169 or (v[0] == v[2] and v[1] == v[3]):
            continue
        out.append(v)
    return np.array(out, np.int8)


def rotated(pat=None):
    """[32, 256, 4]: each test position turned by 2 pi b / 32 and rounded, floor(v + 0.5)"""
    pat = pattern() if pat is None else pat
    out = np.zeros((LF.DIRECTIONS, LF.TESTS, 4), np.int8)
    for b in range(LF.DIRECTIONS):
        a = f64(2 * b) * PI / 32.0
        c, s = np.cos(a), np.sin(a)
        for h in (0, 2):
            x, y = pat[:, h].astype(f64), pat[:, h + 1].astype(f64)
            out[b, :, h] = np.floor((c * x - s * y) + 0.5)
            out[b, :, h + 1] = np.floor((s * x + c * y) + 0.5)
    return out


def bounds():
    a = (2 * np.arange(16) + 1).astype(f64) * PI / 32.0
    return np.stack([np.cos(a), np.sin(a)], 1)


def rotation_margin(pat=None):
    """the smallest distance of a rotated coordinate from a rounding boundary n + 0.5 (exact rotations by multiples of pi / 2 left out)"""
    pat = (pattern() if pat is None else pat).astype(f64)
    best = 1.0
    for b in range(LF.DIRECTIONS):
        if b % 8 == 0:
            continue
        a = f64(2 * b) * PI / 32.0
        c, s = np.cos(a), np.sin(a)
        for h in (0, 2):
            for v in (c * pat[:, h] - s * pat[:, h + 1], s * pat[:, h] + c * pat[:, h + 1]):
                fr = v - np.floor(v)
                best = min(best, float(np.abs(fr - 0.5).min()))
    return best


# ---- features ----
def harris(grey):
    """response per pixel (float32; 0 within 4 of the border)"""
    g = np.asarray(grey, np.uint8).astype(np.int64)
    rows, cols = g.shape
    Ix = np.zeros_like(g); Iy = np.zeros_like(g)
    c = g[1:-1, 1:-1]
    del c
    Ix[1:-1, 1:-1] = 2 * (g[1:-1, 2:] - g[1:-1, :-2]) + (g[:-2, 2:] - g[:-2, :-2]) + (g[2:, 2:] - g[2:, :-2])
    Iy[1:-1, 1:-1] = 2 * (g[2:, 1:-1] - g[:-2, 1:-1]) + (g[2:, :-2] - g[:-2, :-2]) + (g[2:, 2:] - g[:-2, 2:])

    def box7(a):
        out = np.zeros_like(a)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                out[4:rows - 4, 4:cols - 4] += a[4 + dy:rows - 4 + dy, 4 + dx:cols - 4 + dx]
        return out
    sxx, syy, sxy = box7(Ix * Ix), box7(Iy * Iy), box7(Ix * Iy)
    scale = f32(1.0) / (f32(4 * 7) * f32(255.0))
    scale4 = ((scale * scale) * scale) * scale
    a, b = (sxx * syy).astype(f32), (sxy * sxy).astype(f32)
    tr = (sxx + syy).astype(f32)
    r = (a - b) - ((f32(0.04) * tr) * tr) * scale4
    out = np.zeros((rows, cols), f32)
    out[4:rows - 4, 4:cols - 4] = r[4:rows - 4, 4:cols - 4]
    return out


def local_maxima(resp, invdepth):
    """bool map of the keypoint candidates: border, response > 0, beats the 8 neighbours (ties: lower raster index wins), valid inverse depth"""
    rows, cols = resp.shape
    B = LF.BORDER
    ok = np.zeros((rows, cols), bool)
    if rows < 2 * B + 1 or cols < 2 * B + 1:
        return ok
    c = resp[B:rows - B, B:cols - B]
    m = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            nb = resp[B + dy:rows - B + dy, B + dx:cols - B + dx]
            later = dy > 0 or (dy == 0 and dx > 0)       # the neighbour's raster index is larger
            m &= (c > nb) | ((c == nb) & later)
    w = np.asarray(invdepth, f32)[B:rows - B, B:cols - B]
    with np.errstate(invalid="ignore"):
        m &= np.isfinite(w) & (w > 0)
    ok[B:rows - B, B:cols - B] = m
    return ok


def select(resp, ok, max_keypoints):
    """-> [(x, y)] cell-major, each cell's best per_cell by (response descending, raster index ascending)"""
    rows, cols = resp.shape
    cx, cy, k = LF.layout(rows, cols, max_keypoints)
    out = []
    for j in range(cy):
        for i in range(cx):
            ys, xs = np.nonzero(ok[j * LF.CELL:(j + 1) * LF.CELL, i * LF.CELL:(i + 1) * LF.CELL])
            cand = [(-float(resp[j * LF.CELL + y, i * LF.CELL + x]), int((j * LF.CELL + y) * cols + i * LF.CELL + x)) for y, x in zip(ys, xs)]
            out += [(idx % cols, idx // cols) for _, idx in sorted(cand)[:k]]
    return out


def direction(grey, x, y, bnd):
    g = np.asarray(grey, np.uint8).astype(np.int64)
    dy, dx = np.mgrid[-15:16, -15:16]
    disc = dx * dx + dy * dy <= 225
    p = g[y - 15:y + 16, x - 15:x + 16]
    m10, m01 = int((dx * p)[disc].sum()), int((dy * p)[disc].sum())
    upper = m01 > 0 or (m01 == 0 and m10 >= 0)
    mx, my = (f64(m10), f64(m01)) if upper else (-f64(m10), -f64(m01))
    passed = int(np.sum(bnd[:, 0] * my - bnd[:, 1] * mx > 0.0))
    return (passed + (0 if upper else 16)) & 31, m10, m01


def box_sums(grey):
    """5 x 5 box sum centred on every pixel (0 where the box leaves the image)"""
    g = np.asarray(grey, np.uint8).astype(np.int64)
    rows, cols = g.shape
    out = np.zeros_like(g)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            out[2:rows - 2, 2:cols - 2] += g[2 + dy:rows - 2 + dy, 2 + dx:cols - 2 + dx]
    return out


def descriptor(box, x, y, rot_b):
    s1 = box[y + rot_b[:, 1].astype(int), x + rot_b[:, 0].astype(int)]
    s2 = box[y + rot_b[:, 3].astype(int), x + rot_b[:, 2].astype(int)]
    return np.packbits(s1 < s2, bitorder="little")


def lift(x, y, w, Ki):
    """X and the 6 covariance entries in float64, in the header's order of operations"""
    d = f64(f32(1.0) / f32(w))
    px, py, pz = f64(x), f64(y), f64(1.0)
    inv_d = f64(1.0) / d
    s = [f64(f32(0.5) * f32(0.5)), f64(f32(0.5) * f32(0.5)), f64(f32(0.00025) * f32(0.00025))]
    X, J = [], []
    for i in range(3):
        a0, a1, a2 = d * Ki[i, 0], d * Ki[i, 1], d * Ki[i, 2]
        X.append((a0 * px + a1 * py) + a2 * pz)
        mp = (Ki[i, 0] * px + Ki[i, 1] * py) + Ki[i, 2] * pz
        J.append([inv_d * Ki[i, 0], inv_d * Ki[i, 1], -(inv_d * inv_d) * mp])
    cov = [((J[i][0] * s[0]) * J[j][0] + (J[i][1] * s[1]) * J[j][1]) + (J[i][2] * s[2]) * J[j][2] for i in range(3) for j in range(i, 3)]
    return X, cov


def extract(grey, invdepth, K, max_keypoints=1000, tables=None):
    """-> (records KP_DTYPE [max_keypoints] (unused ones zero), count)"""
    rot, bnd = tables if tables is not None else (rotated(), bounds())
    grey = np.asarray(grey, np.uint8); invdepth = np.asarray(invdepth, f32)
    resp = harris(grey)
    pts = select(resp, local_maxima(resp, invdepth), max_keypoints)
    box = box_sums(grey)
    Ki = kinv_numpy(K)
    out = np.zeros(max_keypoints, LF.KP_DTYPE)
    with np.errstate(all="ignore"):
        for k, (x, y) in enumerate(pts):
            b, _, _ = direction(grey, x, y, bnd)
            X, cov = lift(x, y, invdepth[y, x], Ki)
            out[k] = (x, y, resp[y, x], b, descriptor(box, x, y, rot[b]), X, cov)
    return out, len(pts)


# ---- matching ----
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def match(kq, nq, kc, nc, ratio=LF.MATCH_RATIO):
    """2-NN by (distance, candidate index) + ratio test in float32 -> MATCH_DTYPE records in query order"""
    out = []
    if nq > 0 and nc >= 2:
        D = _POP[kq["desc"][:nq, None, :] ^ kc["desc"][None, :nc, :]].sum(2)
        for i in range(nq):
            order = np.argsort(D[i], kind="stable")
            d0, d1 = int(D[i, order[0]]), int(D[i, order[1]])
            if f32(d0) < f32(ratio) * f32(d1):
                out.append((i, int(order[0]), d0, d1))
    return np.array(out, LF.MATCH_DTYPE) if out else np.zeros(0, LF.MATCH_DTYPE)


# ---- RANSAC ----
def sample3(u, m):
    """selectRandomMatches (loop_closer.cpp:555-585) on the list 0 .. m - 1"""
    a = list(range(m))
    size, out = m, []
    for i in range(3):
        idx = int(f64(u[i]) * f64(size))
        out.append(a[idx])
        a[idx] = a[size - 1]
        size -= 1
    return out


def _centred(P):
    c = ((P[0] + P[1]) + P[2]) / 3.0
    return c, P - c


def pose3_svd(Q, Cn):
    """proper rotation of the correlation sum dq dc^T: U diag(1, 1, det(U V^T)) V^T; t = cq - R cc"""
    cq, dq = _centred(np.asarray(Q, f64)); cc, dc = _centred(np.asarray(Cn, f64))
    U, _, Vt = np.linalg.svd(dq.T @ dc)
    R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
    return R, cq - R @ cc


def pose3_horn(Q, Cn):
    """Horn's closed form: the eigenvector of the largest eigenvalue of the 4 x 4 matrix N of the correlation, as a unit quaternion"""
    cq, dq = _centred(np.asarray(Q, f64)); cc, dc = _centred(np.asarray(Cn, f64))
    S = dc.T @ dq      # S_ab = sum c_a q_b: the rotation takes c to q
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])
    w, V = np.linalg.eigh(N)
    q0, qx, qy, qz = V[:, 3]
    R = np.array([[q0 * q0 + qx * qx - qy * qy - qz * qz, 2 * (qx * qy - q0 * qz), 2 * (qx * qz + q0 * qy)],
                  [2 * (qy * qx + q0 * qz), q0 * q0 - qx * qx + qy * qy - qz * qz, 2 * (qy * qz - q0 * qx)],
                  [2 * (qz * qx - q0 * qy), 2 * (qz * qy + q0 * qx), q0 * q0 - qx * qx - qy * qy + qz * qz]])
    return R, cq - R @ cc


def _sym(c6):
    c6 = np.asarray(c6, f64)
    M = np.zeros(c6.shape[:-1] + (3, 3))
    for k, (i, j) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        M[..., i, j] = M[..., j, i] = c6[..., k]
    return M


def errors3d(Xa, ca, Xb, cb, R, t):
    """computeNormalisedError3D for arrays of points: sqrt(v^T (R cov_a R^T + cov_b)^-1 v), v = R X_a + t - X_b"""
    v = Xa @ R.T + t - Xb
    S = R @ _sym(ca) @ R.T + _sym(cb)
    with np.errstate(all="ignore"):
        return np.sqrt(np.einsum("ni,nij,nj->n", v, np.linalg.inv(S), v))


def vote(kq, kc, matches, R, t):
    """both directed errors of every match -> (e_c2q, e_q2c)"""
    Xq, cq = kq["X"][matches["query"]], kq["cov"][matches["query"]]
    Xc, cc = kc["X"][matches["train"]], kc["cov"][matches["train"]]
    return errors3d(Xc, cc, Xq, cq, R, t), errors3d(Xq, cq, Xc, cc, R.T, -R.T @ t)


def ransac(kq, kc, matches, u, th=LF.MAHALANOBIS_TH, guard=1e-6):
    """-> dict(best, inliers, mask, R, t, R_horn, t_horn, fragile).  A hypothesis whose 3 matches share a keypoint is no hypothesis.
    fragile: some hypothesis within one inlier of the best has an error within `guard` of the threshold (the device's rotation comes from
    another factorisation, so such a match may flip)."""
    m = len(matches)
    iters = len(u) // 3
    res = dict(best=-1, inliers=0, mask=np.zeros(m, np.uint8), R=np.full((3, 3), np.nan), t=np.full(3, np.nan), R_horn=None, t_horn=None,
               fragile=False)
    if m < 3:
        return res
    hyp = []
    for h in range(iters):
        s = sample3(u[3 * h:3 * h + 3], m)
        mm = matches[s]
        if len(set(mm["query"])) < 3 or len(set(mm["train"])) < 3:
            continue
        Q, Cn = kq["X"][mm["query"]], kc["X"][mm["train"]]
        R, t = pose3_svd(Q, Cn)
        e1, e2 = vote(kq, kc, matches, R, t)
        inl = (e1 < th) & (e2 < th)
        near = bool(((np.abs(e1 - th) < guard) | (np.abs(e2 - th) < guard)).any())
        hyp.append((h, int(inl.sum()), inl, near, Q, Cn, R, t))
    if not hyp:
        return res
    top = max(c for _, c, *_ in hyp)
    if top == 0:
        return res
    h, c, inl, _, Q, Cn, R, t = next(x for x in hyp if x[1] == top)
    Rh, th_ = pose3_horn(Q, Cn)
    res.update(best=h, inliers=c, mask=inl.astype(np.uint8), R=R, t=t, R_horn=Rh, t_horn=th_,
               fragile=any(near for _, cc_, _, near, *_ in hyp if cc_ >= top - 1))
    return res


# ---- synthetic data ----
def synthetic_pair(r, n_good=60, wrong=0.5, K=(525.0, 525.0, 319.5, 239.5), rows=480, cols=640):
    """random 3-D points seen from two poses with pixel and inverse-depth noise at the lift's sigmas; a share `wrong` of the matches joins
    unrelated keypoints.  Depths are 0.6 - 1.6 m: the lift's Jacobian uses 1 / d where the derivative has d (as the reference writes it), so
    its covariances are right near 1 m only and far too small beyond.  -> (kq, kc records KP_DTYPE, matches MATCH_DTYPE, (R, t) true qTc)"""
    from rgbid.posegraph import _rand_rot
    Ki = kinv_numpy(K)
    R = _rand_rot(r, 0.15); t = r.normal(0, 0.15, 3)
    n_bad = int(round(n_good * wrong / (1.0 - wrong)))
    n = n_good + n_bad

    def observe(Xcam):
        z = Xcam[2]
        x = K[0] * Xcam[0] / z + K[2] + r.normal(0, 0.5)
        y = K[1] * Xcam[1] / z + K[3] + r.normal(0, 0.5)
        w = f32(1.0 / z + r.normal(0, 0.00025))
        return int(np.floor(x + 0.5)), int(np.floor(y + 0.5)), w, x, y

    kq = np.zeros(n, LF.KP_DTYPE); kc = np.zeros(n, LF.KP_DTYPE)
    k = 0
    while k < n:
        Xc = np.array([r.uniform(-0.5, 0.5), r.uniform(-0.4, 0.4), r.uniform(0.6, 1.6)])
        Xq = R @ Xc + t if k < n_good else np.array([r.uniform(-0.5, 0.5), r.uniform(-0.4, 0.4), r.uniform(0.6, 1.6)])
        if Xq[2] < 0.4:
            continue
        oq, oc = observe(Xq), observe(Xc)
        for rec, o in ((kq, oq), (kc, oc)):
            # the noisy sub-pixel position is what a detector would report; the lift sees it through the rounded pixel's ray
            X, cov = lift(o[3], o[4], o[2], Ki)
            rec[k]["x"], rec[k]["y"], rec[k]["X"], rec[k]["cov"] = o[0], o[1], X, cov
        k += 1
    order = r.permutation(n)
    matches = np.zeros(n, LF.MATCH_DTYPE)
    matches["query"], matches["train"] = order, order
    return kq, kc, matches, (R, t)
