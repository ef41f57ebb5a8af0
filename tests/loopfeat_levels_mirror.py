"""Numpy restatement of the multi-level part of the loop-feature contract (include/rgbid_loopfeat.h "levels"): level
geometry, the 11-bit bilinear resize, the budget per level, the depth-at-level-0 predicate, selection with each level's own per_cell and the
level-aware lift, in exact integers / float32 / float64.  Response, local maxima, direction, box sums and descriptor are the single-level
mirror's (tests/loopfeat_mirror.py), applied to a level's image.  The GPU tests compare pyramid, records and aux records with it byte for
byte."""
import math

import numpy as np

from rgbid import loopfeat as LF
from tests import loopfeat_mirror as M
from tests.test_cpu_cloud import kinv_numpy

f32, f64 = np.float32, np.float64


def geometry(rows, cols, levels, scale):
    """-> [(rows_l, cols_l, s_l float32)] of the levels that exist: s_l = (float) pow((double) scale, (double) l), sizes by float division"""
    scale = f32(scale)
    out = []
    for l in range(int(levels)):
        s = f32(math.pow(float(scale), float(l)))
        c, r = int((f32(cols) + f32(0.5)) / s), int((f32(rows) + f32(0.5)) / s)
        if r < 2 * LF.BORDER + 1 or c < 2 * LF.BORDER + 1:
            break
        out.append((r, c, s))
    return out


def budget(rows, cols, max_keypoints, levels, scale):
    """-> [(rows_l, cols_l, cells_x, cells_y, per_cell, s_l)], or None when the slots do not fit into max_keypoints"""
    geo = geometry(rows, cols, levels, scale)
    sd = f64(f32(scale))
    r = f64(1.0) / (sd * sd)
    powers = [f64(1.0)]
    for _ in geo:
        powers.append(powers[-1] * r)
    rL = powers[len(geo)]
    out, slots = [], 0
    for l, (rows_l, cols_l, s) in enumerate(geo):
        n = int(np.floor(f64(max_keypoints) * (((f64(1.0) - r) * powers[l]) / (f64(1.0) - rL))))
        cx, cy = (cols_l + LF.CELL - 1) // LF.CELL, (rows_l + LF.CELL - 1) // LF.CELL
        k = min(max(n // (cx * cy), 1), LF.CELL_MAX)
        out.append((rows_l, cols_l, cx, cy, k, float(s)))
        slots += cx * cy * k
    return out if slots <= max_keypoints else None


def resize_table(src, dst):
    """(x0, w1) int32 [dst] of one axis"""
    d = np.arange(dst, dtype=f64)
    fx = (d + 0.5) * (f64(src) / f64(dst)) - 0.5
    fl = np.floor(fx)
    x0 = fl.astype(np.int64)
    w1 = np.floor((fx - fl) * 2048.0 + 0.5).astype(np.int64)
    low, high = x0 < 0, x0 >= src - 1
    x0 = np.where(low, 0, np.where(high, src - 1, x0))
    w1 = np.where(low | high, 0, w1)
    return x0.astype(np.int32), w1.astype(np.int32)


def resize(img, drows, dcols):
    """one level from the one below, in integers"""
    g = np.asarray(img, np.uint8).astype(np.int64)
    srows, scols = g.shape
    x0, w1x = [a.astype(np.int64) for a in resize_table(scols, dcols)]
    y0, w1y = [a.astype(np.int64) for a in resize_table(srows, drows)]
    x1, y1 = np.minimum(x0 + 1, scols - 1), np.minimum(y0 + 1, srows - 1)
    w0x, w0y = 2048 - w1x, 2048 - w1y
    top = w0x[None, :] * g[y0][:, x0] + w1x[None, :] * g[y0][:, x1]
    bot = w0x[None, :] * g[y1][:, x0] + w1x[None, :] * g[y1][:, x1]
    v = (w0y[:, None] * top + w1y[:, None] * bot + (1 << 21)) >> 22
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def pyramid(grey, geo):
    """[level images]: level 0 is the input, each further one is resized from the one before"""
    out = [np.asarray(grey, np.uint8)]
    for rows_l, cols_l, *_ in geo[1:]:
        out.append(resize(out[-1], rows_l, cols_l))
    return out


def pixel0(v, s):
    """(float product v s_l, the level-0 pixel (int) ((double) product + 0.5)) of level coordinates v (array)"""
    p = np.asarray(v).astype(f32) * f32(s)
    return p, (p.astype(f64) + 0.5).astype(np.int64)


def keypoint_map(resp, invdepth0, s):
    """the single-level predicate on the level's response, with the depth read at the level-0 pixel"""
    rows_l, cols_l = resp.shape
    rows, cols = invdepth0.shape
    _, X0 = pixel0(np.arange(cols_l), s)
    _, Y0 = pixel0(np.arange(rows_l), s)
    inside = (Y0 < rows)[:, None] & (X0 < cols)[None, :]
    w = np.asarray(invdepth0, f32)[np.minimum(Y0, rows - 1)][:, np.minimum(X0, cols - 1)]
    with np.errstate(invalid="ignore"):
        valid = inside & np.isfinite(w) & (w > 0)
    return M.local_maxima(resp, np.ones((rows_l, cols_l), f32)) & valid


def select(resp, ok, cells_x, cells_y, per_cell):
    """-> [(x, y)] cell-major, each cell's best per_cell by (response descending, raster index ascending)"""
    cols = resp.shape[1]
    out = []
    for j in range(cells_y):
        for i in range(cells_x):
            ys, xs = np.nonzero(ok[j * LF.CELL:(j + 1) * LF.CELL, i * LF.CELL:(i + 1) * LF.CELL])
            cand = [(-float(resp[j * LF.CELL + y, i * LF.CELL + x]), int((j * LF.CELL + y) * cols + i * LF.CELL + x)) for y, x in zip(ys, xs)]
            out += [(idx % cols, idx // cols) for _, idx in sorted(cand)[:per_cell]]
    return out


def lift(px, py, w, Ki, s):
    """X and the 6 covariance entries in float64: p = ((double) px, (double) py, 1), pixel variances (double) (((s s) 0.5f) 0.5f)"""
    s = f32(s)
    d = f64(f32(1.0) / f32(w))
    px, py, pz = f64(f32(px)), f64(f32(py)), f64(1.0)
    inv_d = f64(1.0) / d
    var = f64(((s * s) * f32(0.5)) * f32(0.5))
    sg = [var, var, f64(f32(0.00025) * f32(0.00025))]
    X, J = [], []
    for i in range(3):
        a0, a1, a2 = d * Ki[i, 0], d * Ki[i, 1], d * Ki[i, 2]
        X.append((a0 * px + a1 * py) + a2 * pz)
        mp = (Ki[i, 0] * px + Ki[i, 1] * py) + Ki[i, 2] * pz
        J.append([inv_d * Ki[i, 0], inv_d * Ki[i, 1], -(inv_d * inv_d) * mp])
    cov = [((J[i][0] * sg[0]) * J[j][0] + (J[i][1] * sg[1]) * J[j][1]) + (J[i][2] * sg[2]) * J[j][2] for i in range(3) for j in range(i, 3)]
    return X, cov


def extract(grey, invdepth, K, max_keypoints=1000, levels=1, scale=1.2, tables=None):
    """-> (records KP_DTYPE [max_keypoints], aux AUX_DTYPE [max_keypoints] (unused ones zero), count); level-major, cell-major, rank"""
    rot, bnd = tables if tables is not None else (M.rotated(), M.bounds())
    grey = np.asarray(grey, np.uint8); invdepth = np.asarray(invdepth, f32)
    plan = budget(grey.shape[0], grey.shape[1], max_keypoints, levels, scale)
    assert plan is not None, "the levels' slots do not fit into max_keypoints"
    Ki = kinv_numpy(K)
    out = np.zeros(max_keypoints, LF.KP_DTYPE)
    aux = np.zeros(max_keypoints, LF.AUX_DTYPE)
    k = 0
    with np.errstate(all="ignore"):
        for level, (img, (_, _, cx, cy, per_cell, s)) in enumerate(zip(pyramid(grey, plan), plan)):
            resp = M.harris(img)
            box = M.box_sums(img)
            for x, y in select(resp, keypoint_map(resp, invdepth, s), cx, cy, per_cell):
                (px, X0), (py, Y0) = pixel0(x, s), pixel0(y, s)
                b, _, _ = M.direction(img, x, y, bnd)
                X, cov = lift(px, py, invdepth[int(Y0), int(X0)], Ki, s)
                out[k] = (int(X0), int(Y0), resp[y, x], b, M.descriptor(box, x, y, rot[b]), X, cov)
                aux[k] = (px, py, x, y, level)
                k += 1
    return out, aux, k


# ---- the scale-change pair of the issue ----
PAIR_K = (262.5, 262.5, 159.5, 119.5)
PAIR_ROWS, PAIR_COLS = 240, 320


def scale_change_pair(tz=0.75):
    """the default synthetic scene rendered noise-free at 320 x 240 from t = (0.05, -0.03, 0) and from the same point moved tz closer, identity
    rotation -> ([grey a, grey b] uint8 as a keyframe's grey image is formed, [inverse depth a, b] = 1000.f / round(mm), [colors a, b],
    (R, t) of the far view's points in the near view's frame: X_b = X_a - (0, 0, tz))"""
    from rgbid import synth
    from rgbid.posegraph import grey_from_colors
    scene = synth.Scene()
    greys, ws, colors = [], [], []
    for t in ((0.05, -0.03, 0.0), (0.05, -0.03, float(tz))):
        d_mm, rgb8 = synth.make_frame(scene, np.eye(3), np.array(t), PAIR_K, PAIR_ROWS, PAIR_COLS, noise=False, dropout=0.0)
        c = rgb8.cpu().numpy()
        mm = d_mm.cpu().numpy().astype(f32)
        with np.errstate(divide="ignore"):
            ws.append(np.where(mm > 0, f32(1000.0) / mm, f32(0.0)).astype(f32))
        colors.append(c)
        greys.append(grey_from_colors(c))
    return greys, ws, colors, (np.eye(3), np.array([0.0, 0.0, -float(tz)]))


def appearance_gate(ka, na, kb, nb, rows=PAIR_ROWS, cols=PAIR_COLS):
    """mirror match (query b, candidate a) + RANSAC at the reference's iteration count and seed + the host gate
    -> dict(matches, ransac result, ok, inliers, hulls)"""
    m = M.match(kb, nb, ka, na)
    u = LF.uniform_draws(LF.num_iters())
    res = M.ransac(kb, ka, m, u)
    ok, inl, hq, hc = LF.gate(kb, ka, m, res["mask"], rows, cols) if res["best"] >= 0 else (False, 0, 0.0, 0.0)
    return dict(matches=m, ransac=res, u=u, ok=ok, inliers=inl, hull_query=hq, hull_candidate=hc)
