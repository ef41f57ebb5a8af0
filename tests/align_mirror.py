"""numpy restatement of steps 24 - 33 of the TSDF volume's contract (include/rgbid_tsdf_align.h): the judge of
k_tsdf_align_system and k_tsdf_align_solve in csrc/kernels_tsdf.hip.  Every float32 value is formed by np.float32 operations and every
double by float64 operations in exactly the order of the header; the sums follow the header's fixed tree; integers and comparisons decide.
`align` is vectorised over the pixels of a level; `align_loop` is the plain scalar loop of the same contract that the CPU tests hold it
against."""
import math

import numpy as np

from tests import raycast_mirror as RM
from tests.tsdf_mirror import measured_depth

F = np.float32
D = np.float64
RUNNING, CONVERGED, FEW, SINGULAR = 0, 1, 2, 3
STATUS_NAMES = ("running", "converged", "few", "singular")
TERMS = 28
NAN_BITS = np.uint64(0x7FFFFFFFFFFFFFFF)                         # RGBID_TSDF_ALIGN_NAN_BITS
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]          # the 21 products of step 27, row-major
STRIDES = (1, 2, 4, 8)
RESULT_DTYPE = np.dtype([("pose", "<f8", (12,)), ("status", "<i4"), ("iterations", "<i4"), ("used", "<u4", (2,)), ("sums", "<f8", (2, TERMS))])
assert RESULT_DTYPE.itemsize == 560


def lattice(rows, cols, stride):
    """step 25: the lattice's (rows, cols)"""
    return (rows + stride - 1) // stride, (cols + stride - 1) // stride


def pose32(pose):
    """step 24: the float32 roundings of the 12 doubles"""
    with np.errstate(over="ignore"):
        return np.asarray(pose, D).astype(F)


def pixel_values(vol, plane, m, K, rows, cols, stride, z_min, z_max, min_weight, huber):
    """steps 25 and 26 for the lattice of one view at the float32 pose m -> dict of arrays over [lattice rows, lattice cols]: used,
    measured, z, g (3), defined, f, G (3), J (6), w, a (6)"""
    fx, fy, cx, cy = (F(v) for v in K)
    lh, lw = lattice(rows, cols, stride)
    pu, pv = np.arange(lw) * stride, np.arange(lh) * stride
    meas, z = measured_depth(np.asarray(plane, F)[pv[:, None], pu[None, :]])
    dx, dy = ((pu.astype(F) - cx) / fx)[None, :], ((pv.astype(F) - cy) / fy)[:, None]
    with np.errstate(all="ignore"):
        gate = meas & (z >= F(z_min)) & (z <= F(z_max))
        xc, yc = dx * z, dy * z
        p = [((m[3 * i] * xc + m[3 * i + 1] * yc) + m[3 * i + 2] * z) + m[9 + i] for i in range(3)]
        g = [(p[i] - vol.origin[i]) / vol.voxel for i in range(3)]
        defined, base, fx_, fy_, fz_ = RM.cell(vol, g[0].reshape(-1), g[1].reshape(-1), g[2].reshape(-1), min_weight)
        Dv = vol.D.reshape(-1)
        d = [Dv[base + o] for o in RM.corner_offsets(vol)]
        f = RM.trilinear(d, fx_, fy_, fz_).reshape(lh, lw)
        G = [(c / vol.voxel).reshape(lh, lw) for c in RM.gradient(d, fx_, fy_, fz_)]
        defined = defined.reshape(lh, lw)
        used = gate & defined & (np.abs(f) < vol.trunc)
        J = [G[0], G[1], G[2], p[1] * G[2] - p[2] * G[1], p[2] * G[0] - p[0] * G[2], p[0] * G[1] - p[1] * G[0]]
        w = np.where(np.abs(f) <= F(huber), F(1), F(huber) / np.abs(f))
        a = [w * j for j in J]
    assert all(x.dtype == F for x in p + g + G + J + a + [f, w, z])
    return dict(used=used, measured=meas, gate=gate, z=z, p=p, g=g, defined=defined, f=f, G=G, J=J, w=w, a=a)


def terms_of(px):
    """step 27 -> float64 [28, lattice rows, lattice cols], +0.0 where the pixel is not used"""
    with np.errstate(all="ignore"):
        a, J, f = [x.astype(D) for x in px["a"]], [x.astype(D) for x in px["J"]], px["f"].astype(D)
        t = [a[i] * J[j] for i, j in PAIRS] + [a[i] * f for i in range(6)] + [(px["w"] * px["f"]).astype(D) * f]
    return np.where(px["used"][None], np.stack(t), D(0))


def tree64(v):
    """step 28: [..., 64] -> [...]: v[l] + v[l ^ 1], then across bit 1, ... bit 5"""
    assert v.shape[-1] == 64
    with np.errstate(all="ignore"):
        for _ in range(6):
            v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def tile_lanes(x):
    """[..., lattice rows, lattice cols] -> [..., tiles, 64]: 8 x 8 tiles in raster order, lane (ly & 7) 8 + (lx & 7), zeros outside"""
    lh, lw = x.shape[-2:]
    ty, tx = (lh + 7) // 8, (lw + 7) // 8
    pad = np.zeros(x.shape[:-2] + (ty * 8, tx * 8), x.dtype)
    pad[..., :lh, :lw] = x
    lead = pad.shape[:-2]
    k = len(lead)
    return pad.reshape(lead + (ty, 8, tx, 8)).transpose(tuple(range(k)) + (k, k + 2, k + 1, k + 3)).reshape(lead + (ty * tx, 64))


def reduce_tiles(s):
    """step 28's upper tree: [..., n] -> [...]: while more than one value is left, pad with +0.0 to a multiple of 64 and tree64 each 64"""
    while s.shape[-1] > 1:
        n = s.shape[-1]
        pad = np.zeros(s.shape[:-1] + ((n + 63) // 64 * 64,), s.dtype)
        pad[..., :n] = s
        s = tree64(pad.reshape(s.shape[:-1] + (-1, 64)))
    return s[..., 0]


def system(vol, plane, m, K, rows, cols, stride, z_min, z_max, min_weight, huber):
    """steps 25 - 28 -> (used count, the 28 sums as float64)"""
    px = pixel_values(vol, plane, m, K, rows, cols, stride, z_min, z_max, min_weight, huber)
    return int(px["used"].sum()), reduce_tiles(tree64(tile_lanes(terms_of(px))))


def unpack(sums):
    """the 28 sums -> (H float64 [6, 6] symmetric, b [6], error)"""
    H = np.zeros((6, 6), D)
    for k, (i, j) in enumerate(PAIRS):
        H[i, j] = H[j, i] = sums[k]
    return H, np.array(sums[21:27], D), float(sums[27])


def solve(sums, damping):
    """step 30 in Python floats (IEEE doubles, no fused operation) -> delta as a list of 6, or None: SINGULAR"""
    Hm, b, _ = unpack(sums)
    H = [[float(Hm[i, j]) for j in range(6)] for i in range(6)]
    b = [float(x) for x in b]
    damp = 1.0 + float(damping)
    for j in range(6):
        H[j][j] = H[j][j] * damp
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = H[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not (s > 0.0 and math.isfinite(s)):
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            s = H[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        s = -b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s / L[i][i]
    if not all(math.isfinite(v) for v in x):
        return None
    return x


def update(pose, delta):
    """step 31 in Python floats: pose = the 12 doubles R00 .. R22 tx ty tz, delta = (v, omega) -> the new 12 doubles"""
    R, t = [float(x) for x in pose[:9]], [float(x) for x in pose[9:]]
    v = delta[:3]
    hx, hy, hz = delta[3] / 2.0, delta[4] / 2.0, delta[5] / 2.0
    n = math.sqrt(1.0 + ((hx * hx + hy * hy) + hz * hz))
    qw, qx, qy, qz = 1.0 / n, hx / n, hy / n, hz / n
    xx, yy, zz, xy, xz, yz, wx, wy, wz = qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz, qw * qx, qw * qy, qw * qz
    dR = [1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy),
          2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx),
          2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]
    Rn = [(dR[3 * i] * R[j] + dR[3 * i + 1] * R[3 + j]) + dR[3 * i + 2] * R[6 + j] for i in range(3) for j in range(3)]
    tn = [((dR[3 * i] * t[0] + dR[3 * i + 1] * t[1]) + dR[3 * i + 2] * t[2]) + v[i] for i in range(3)]
    return np.array(Rn + tn, D)


def one_nan(a):
    """step 33: every NaN of a float64 array -> the bits NAN_BITS"""
    b = np.ascontiguousarray(a, D).copy()
    b.view(np.uint64)[np.isnan(b)] = NAN_BITS
    return b


def _run(system_fn, V, R, t, levels, damping, eps, min_pixels):
    out = np.zeros(V, RESULT_DTYPE)
    for v in range(V):
        pose = np.concatenate([R[v].reshape(9), t[v]]).astype(D)
        status, its = RUNNING, 0
        for stride, iters in levels:
            if status == CONVERGED:
                status = RUNNING
            for _ in range(iters):
                if status != RUNNING:
                    break
                used, sums = system_fn(v, pose32(pose), stride)
                if its == 0:
                    out[v]["used"][0], out[v]["sums"][0] = used, one_nan(sums)
                out[v]["used"][1], out[v]["sums"][1] = used, one_nan(sums)
                its += 1
                if used < min_pixels:
                    status = FEW
                    break
                delta = solve(sums, damping)
                if delta is None:
                    status = SINGULAR
                    break
                pose = update(pose, delta)
                if max(abs(x) for x in delta) < eps:
                    status = CONVERGED
        out[v]["pose"], out[v]["status"], out[v]["iterations"] = one_nan(pose), status, its
    return out


def align(vol, planes, R, t, K, rows, cols, levels, huber=None, damping=0.0, eps=1e-6, min_pixels=64, min_weight=1, z_min=0.05, z_max=20.0):
    """steps 24 - 33 for V views -> the result records (RESULT_DTYPE [V]) as the device writes them"""
    R = np.asarray(R, D).reshape(-1, 3, 3); t = np.asarray(t, D).reshape(-1, 3)
    huber = vol.trunc if huber is None else huber
    fn = lambda v, m, stride: system(vol, planes[v], m, K, rows, cols, stride, z_min, z_max, min_weight, huber)
    return _run(fn, len(R), R, t, levels, damping, eps, min_pixels)


def as_dict(res):
    """the records as Volume.align returns them"""
    H = np.zeros((len(res), 2, 6, 6), D)
    for k, (i, j) in enumerate(PAIRS):
        H[:, :, i, j] = H[:, :, j, i] = res["sums"][:, :, k]
    return dict(R=res["pose"][:, :9].reshape(-1, 3, 3).copy(), t=res["pose"][:, 9:].copy(), status=res["status"].copy(),
                iterations=res["iterations"].copy(), used=res["used"].copy(), H=H, b=res["sums"][:, :, 21:27].copy(),
                error=res["sums"][:, :, 27].copy())


# ---- the scalar loop ----------------------------------------------------------------------------------------------------------------------
def _pixel_loop(vol, plane, m, K, pu, pv, z_min, z_max, min_weight, huber):
    """steps 26 and 27 for one pixel -> the 28 terms as Python floats, or None when the pixel is not used"""
    fx, fy, cx, cy = (F(v) for v in K)
    mm = F(plane[pv, pu])
    if not (np.isfinite(mm) and mm > 0):
        return None
    z = F(F(1) / mm)
    if not np.isfinite(z) or not (F(z_min) <= z <= F(z_max)):
        return None
    dx, dy = F(F(F(pu) - cx) / fx), F(F(F(pv) - cy) / fy)
    xc, yc = F(dx * z), F(dy * z)
    p = [F(F(F(F(m[3 * i] * xc) + F(m[3 * i + 1] * yc)) + F(m[3 * i + 2] * z)) + m[9 + i]) for i in range(3)]
    g = [F(F(p[i] - vol.origin[i]) / vol.voxel) for i in range(3)]
    s = RM._sample_loop(vol, g[0], g[1], g[2], min_weight)
    if s is None:
        return None
    _, fx_, fy_, fz_, d = s
    f = RM._tri_loop(d, fx_, fy_, fz_)
    if not abs(f) < vol.trunc:
        return None
    l = RM._l
    lx = [l(d[2 * q], d[2 * q + 1], fx_) for q in range(4)]
    G = [F(l(l(F(d[1] - d[0]), F(d[3] - d[2]), fy_), l(F(d[5] - d[4]), F(d[7] - d[6]), fy_), fz_) / vol.voxel),
         F(l(F(lx[1] - lx[0]), F(lx[3] - lx[2]), fz_) / vol.voxel),
         F(F(l(lx[2], lx[3], fy_) - l(lx[0], lx[1], fy_)) / vol.voxel)]
    J = G + [F(F(p[1] * G[2]) - F(p[2] * G[1])), F(F(p[2] * G[0]) - F(p[0] * G[2])), F(F(p[0] * G[1]) - F(p[1] * G[0]))]
    w = F(1) if abs(f) <= F(huber) else F(F(huber) / abs(f))
    a = [F(w * j) for j in J]
    return [float(a[i]) * float(J[j]) for i, j in PAIRS] + [float(a[i]) * float(f) for i in range(6)] + [float(F(w * f)) * float(f)]


def tree64_loop(v):
    """step 28's tree over a list of 64 Python floats, as an explicit loop over the lanes"""
    v = list(v)
    assert len(v) == 64
    for bit in range(6):
        v = [v[l] + v[l ^ (1 << bit)] for l in range(64)]
    assert all(x == v[0] or (x != x and v[0] != v[0]) for x in v)          # every lane holds the sum
    return v[0]


def reduce_loop(s):
    s = list(s)
    while len(s) > 1:
        s = s + [0.0] * (-len(s) % 64)
        s = [tree64_loop(s[k:k + 64]) for k in range(0, len(s), 64)]
    return s[0]


def system_loop(vol, plane, m, K, rows, cols, stride, z_min, z_max, min_weight, huber):
    lh, lw = lattice(rows, cols, stride)
    ty, tx = (lh + 7) // 8, (lw + 7) // 8
    used, tiles = 0, []
    with np.errstate(all="ignore"):
        for tj in range(ty):
            for ti in range(tx):
                lanes = [[0.0] * 64 for _ in range(TERMS)]
                for lane in range(64):
                    lx, ly = ti * 8 + (lane & 7), tj * 8 + (lane >> 3)
                    if lx >= lw or ly >= lh:
                        continue
                    tm = _pixel_loop(vol, plane, m, K, lx * stride, ly * stride, z_min, z_max, min_weight, huber)
                    if tm is None:
                        continue
                    used += 1
                    for k in range(TERMS):
                        lanes[k][lane] = tm[k]
                tiles.append([tree64_loop(lanes[k]) for k in range(TERMS)])
    return used, np.array([reduce_loop([tl[k] for tl in tiles]) for k in range(TERMS)], D)


def align_loop(vol, planes, R, t, K, rows, cols, levels, huber=None, damping=0.0, eps=1e-6, min_pixels=64, min_weight=1, z_min=0.05, z_max=20.0):
    R = np.asarray(R, D).reshape(-1, 3, 3); t = np.asarray(t, D).reshape(-1, 3)
    huber = vol.trunc if huber is None else huber
    fn = lambda v, m, stride: system_loop(vol, np.asarray(planes[v], F), m, K, rows, cols, stride, z_min, z_max, min_weight, huber)
    return _run(fn, len(R), R, t, levels, damping, eps, min_pixels)


# ---- what the tools print -----------------------------------------------------------------------------------------------------------------
def correction(R0, t0, R1, t1):
    """the rotation angle (rad) and the translation (m) between two world poses"""
    dR = np.asarray(R1, D) @ np.asarray(R0, D).T
    c = min(1.0, max(-1.0, (np.trace(dR) - 1.0) / 2.0))
    return math.acos(c), float(np.linalg.norm(np.asarray(t1, D) - np.asarray(t0, D)))
