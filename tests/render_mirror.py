"""numpy restatement of the map renderer's contract (include/rgbid_render.h): the judge of csrc/kernels_render.hip.
Every float32 value is formed by np.float32 operations in exactly the order of the header (no `@`, no fused operation); the winner of a
pixel is the minimum of uint64 keys (bits of Z << 32 | record index), reduced with np.minimum.at."""
import numpy as np

F = np.float32
EMPTY = np.uint32(0xFFFFFFFF)
NAN_BITS = np.uint32(0x7FFFFFFF)
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def pose_cw(R, t):
    """step 1: world pose (double) -> r00 .. r22, tx, ty, tz as float32: R_CW = R_WC^T, t_CW[i] = -((R[0][i] t0 + R[1][i] t1) + R[2][i] t2)"""
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3)
    out = np.empty(12, F)
    with np.errstate(over="ignore"):
        for i in range(3):
            for j in range(3):
                out[3 * i + j] = F(R[j, i])
            out[9 + i] = F(-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]))
    return out


def rot_row(m, x, y, z):
    """(m0 x + m1 y) + m2 z in float32, one rounding per operation"""
    return (m[0] * x + m[1] * y) + m[2] * z


def one_nan(a):
    """every NaN of a float32 array -> the bits NAN_BITS"""
    b = np.ascontiguousarray(a, F).copy()
    b.view(np.uint32)[np.isnan(b)] = NAN_BITS
    return b


def visible(p, m, K, rows, cols, s, z_min, z_max):
    """steps 2 - 5 for one view: -> (record indices, pu, pv as int64, Z float32) of the records that write somewhere"""
    fx, fy, cx, cy = (F(v) for v in K)
    x, y, z = p["x"], p["y"], p["z"]
    with np.errstate(all="ignore"):
        X = rot_row(m[0:3], x, y, z) + m[9]
        Y = rot_row(m[3:6], x, y, z) + m[10]
        Z = rot_row(m[6:9], x, y, z) + m[11]
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(Z) & (Z >= F(z_min)) & (Z <= F(z_max))
        pu = np.floor((fx * (X / Z) + cx) + F(0.5))
        pv = np.floor((fy * (Y / Z) + cy) + F(0.5))
        ok &= (pu >= F(-s)) & (pu <= F(cols - 1 + s)) & (pv >= F(-s)) & (pv <= F(rows - 1 + s))     # float compare; NaN and inf fail
    i = np.nonzero(ok)[0]
    assert X.dtype == Y.dtype == Z.dtype == pu.dtype == F
    return i, pu[i].astype(np.int64), pv[i].astype(np.int64), Z[i]


def view_keys(p, m, K, rows, cols, s, z_min, z_max):
    """steps 2 - 7 for one view: -> uint64 [rows, cols] keys, EMPTY_KEY where nothing was written"""
    i, pu, pv, Z = visible(p, m, K, rows, cols, s, z_min, z_max)
    keys = np.full(rows * cols, EMPTY_KEY, np.uint64)
    key = (Z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)
    for dy in range(-s, s + 1):
        for dx in range(-s, s + 1):
            u, v = pu + dx, pv + dy
            inside = (u >= 0) & (u < cols) & (v >= 0) & (v < rows)
            np.minimum.at(keys, (v[inside] * cols + u[inside]), key[inside])
    return keys.reshape(rows, cols)


def resolve(p, m, keys):
    """step 8: keys [rows, cols] -> index uint32, depth float32, colour uint8 [rows, cols, 3], normal float32 [3, rows, cols]"""
    rows, cols = keys.shape
    empty = keys == EMPTY_KEY
    index = np.where(empty, EMPTY, (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)).astype(np.uint32)
    depth = (keys >> np.uint64(32)).astype(np.uint32)
    depth[empty] = NAN_BITS
    depth = depth.view(F)
    w = p[np.where(empty, 0, index)] if len(p) else np.zeros((rows, cols), p.dtype)
    colour = np.stack([w["r"], w["g"], w["b"]], -1).astype(np.uint8)
    colour[empty] = 0
    with np.errstate(all="ignore"):
        normal = np.stack([rot_row(m[3 * a:3 * a + 3], w["nx"], w["ny"], w["nz"]) for a in range(3)]).astype(F)
    normal[:, empty] = np.nan
    return index, depth, colour, one_nan(normal)


def render_numpy(p, R, t, K, rows, cols, s=1, z_min=0.05, z_max=20.0):
    """records p (structured, rgbid.cloud.POINT_DTYPE), world poses R [V, 3, 3], t [V, 3] -> dict of index uint32 [V, rows, cols], depth
    float32 [V, rows, cols], colour uint8 [V, rows, cols, 3], normal float32 [V, 3, rows, cols]"""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3); t = np.asarray(t, np.float64).reshape(-1, 3)
    out = {"index": [], "depth": [], "colour": [], "normal": []}
    for v in range(len(R)):
        m = pose_cw(R[v], t[v])
        planes = resolve(p, m, view_keys(p, m, K, rows, cols, s, z_min, z_max))
        for name, plane in zip(("index", "depth", "colour", "normal"), planes):
            out[name].append(plane)
    return {k: np.stack(v) for k, v in out.items()}


def render_bruteforce(p, R, t, K, rows, cols, s, z_min, z_max):
    """An independent restatement for small inputs: per pixel, a loop over all records taking min over tuples (Z, index); it shares the
    projection of `visible` but not the key packing or the scatter.  -> (index int64 [rows, cols], -1 empty; depth float32, NaN empty)"""
    m = pose_cw(R, t)
    i, pu, pv, Z = visible(p, m, K, rows, cols, s, z_min, z_max)
    index = np.full((rows, cols), -1, np.int64)
    depth = np.full((rows, cols), np.nan, F)
    for y in range(rows):
        for x in range(cols):
            best = None
            for k in range(len(i)):
                if abs(int(pu[k]) - x) <= s and abs(int(pv[k]) - y) <= s:
                    cand = (float(Z[k]), int(i[k]))
                    best = cand if best is None else min(best, cand)
            if best is not None:
                depth[y, x], index[y, x] = F(best[0]), best[1]
    return index, depth
