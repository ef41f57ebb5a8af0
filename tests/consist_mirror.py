"""numpy restatement of the consistency filter's contract (include/rgbid_consist.h): the judge of
csrc/kernels_consist.hip.  Every float32 value is formed by np.float32 operations in exactly the order of the header (no `@`, no fused
operation); the decision per (record, view) is made of booleans and the counts are integers.  `consist_numpy` is vectorised over the
records; `consist_loop` is the plain scalar triple loop of the same contract that the CPU tests hold it against."""
import numpy as np

from tests.render_mirror import pose_cw, rot_row

F = np.float32


def measured_depth(m):
    """step 7 for an array of inverse depths: -> (measured, z_m); measured iff m is finite and > 0 and 1.f / m is finite"""
    m = np.asarray(m, F)
    with np.errstate(all="ignore"):
        zm = F(1) / m
        ok = np.isfinite(m) & (m > 0) & np.isfinite(zm)
    return ok, zm


def view_verdicts(p, m, plane, K, w, tol_rel, tol_abs, z_min, z_max, own=None):
    """steps 2 - 8 for one view: -> (supports, contradicts, gated) as bool [n]; own = (first, last) of the records the view owns"""
    rows, cols = plane.shape
    fx, fy, cx, cy = (F(v) for v in K)
    x, y, z = p["x"], p["y"], p["z"]
    n = len(p)
    with np.errstate(all="ignore"):
        X = rot_row(m[0:3], x, y, z) + m[9]
        Y = rot_row(m[3:6], x, y, z) + m[10]
        Z = rot_row(m[6:9], x, y, z) + m[11]
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(Z) & (Z >= F(z_min)) & (Z <= F(z_max))
        pu = np.floor((fx * (X / Z) + cx) + F(0.5))
        pv = np.floor((fy * (Y / Z) + cy) + F(0.5))
        ok &= (pu >= F(0)) & (pu <= F(cols - 1)) & (pv >= F(0)) & (pv <= F(rows - 1))     # float compare; NaN and inf fail
        d = F(tol_rel) * Z + F(tol_abs)
    assert X.dtype == Y.dtype == Z.dtype == pu.dtype == d.dtype == F
    if own is not None:
        ok[int(own[0]):int(own[1])] = False
    i = np.nonzero(ok)[0]
    iu, iv, Zi, di = pu[i].astype(np.int64), pv[i].astype(np.int64), Z[i], d[i]
    any_measured = np.zeros(len(i), bool); supported = np.zeros(len(i), bool); behind = np.ones(len(i), bool)
    for dy in range(-w, w + 1):
        for dx in range(-w, w + 1):
            u, v = iu + dx, iv + dy
            inside = (u >= 0) & (u < cols) & (v >= 0) & (v < rows)
            meas, zm = measured_depth(plane[np.where(inside, v, 0), np.where(inside, u, 0)])
            meas &= inside
            with np.errstate(all="ignore"):
                e = zm - Zi
                supported |= meas & (np.abs(e) <= di)
                behind &= ~meas | (e > di)
            any_measured |= meas
    sup, con = np.zeros(n, bool), np.zeros(n, bool)
    sup[i] = supported
    con[i] = ~supported & any_measured & behind
    return sup, con, ok


def consist_numpy(p, offsets, planes, R, t, K, tol_rel=0.02, tol_abs=0.0, window=1, min_support=0, max_conflicts=0, z_min=0.05, z_max=20.0):
    """records p (structured, rgbid.cloud.POINT_DTYPE), offsets [V + 1] or None, planes [V][rows, cols] float32, world poses R [V, 3, 3],
    t [V, 3] -> (counts uint32 [n] = support | conflicts << 16, keep bool [n], kept records, pairs past the gates)"""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3); t = np.asarray(t, np.float64).reshape(-1, 3)
    n = len(p)
    support, conflicts, pairs = np.zeros(n, np.uint32), np.zeros(n, np.uint32), 0
    for v in range(len(R)):
        own = None if offsets is None else (offsets[v], offsets[v + 1])
        sup, con, gated = view_verdicts(p, pose_cw(R[v], t[v]), np.asarray(planes[v], F), K, window, tol_rel, tol_abs, z_min, z_max, own)
        support += sup; conflicts += con; pairs += int(gated.sum())
    part = np.isfinite(p["x"]) & np.isfinite(p["y"]) & np.isfinite(p["z"])
    assert not support[~part].any() and not conflicts[~part].any()
    keep = part & (support >= min_support) & (conflicts <= max_conflicts)
    return support | (conflicts << np.uint32(16)), keep, p[keep], pairs


def consist_loop(p, offsets, planes, R, t, K, tol_rel, tol_abs, window, z_min, z_max):
    """the contract as a scalar loop over views, records and window pixels -> (support, conflicts) as int arrays"""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3); t = np.asarray(t, np.float64).reshape(-1, 3)
    fx, fy, cx, cy = (F(v) for v in K)
    n = len(p)
    support, conflicts = np.zeros(n, np.int64), np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for v in range(len(R)):
            m = pose_cw(R[v], t[v])
            plane = np.asarray(planes[v], F)
            rows, cols = plane.shape
            for i in range(n):
                if offsets is not None and offsets[v] <= i < offsets[v + 1]:
                    continue
                x, y, z = p["x"][i], p["y"][i], p["z"][i]
                if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
                    continue
                X = F(F(F(m[0] * x) + F(m[1] * y)) + F(m[2] * z)) + m[9]
                Y = F(F(F(m[3] * x) + F(m[4] * y)) + F(m[5] * z)) + m[10]
                Z = F(F(F(m[6] * x) + F(m[7] * y)) + F(m[8] * z)) + m[11]
                if not (F(z_min) <= Z <= F(z_max)):
                    continue
                pu = np.floor(F(F(fx * F(X / Z)) + cx) + F(0.5))
                pv = np.floor(F(F(fy * F(Y / Z)) + cy) + F(0.5))
                if not (0 <= pu <= cols - 1 and 0 <= pv <= rows - 1):
                    continue
                pu, pv = int(pu), int(pv)
                d = F(F(F(tol_rel) * Z) + F(tol_abs))
                supported, measured, behind = False, 0, 0
                for yy in range(max(pv - window, 0), min(pv + window, rows - 1) + 1):
                    for xx in range(max(pu - window, 0), min(pu + window, cols - 1) + 1):
                        iD = plane[yy, xx]
                        if not (np.isfinite(iD) and iD > 0):
                            continue
                        zm = F(F(1) / iD)
                        if not np.isfinite(zm):
                            continue
                        e = F(zm - Z)
                        measured += 1
                        supported |= bool(abs(e) <= d)
                        behind += bool(e > d)
                if supported:
                    support[i] += 1
                elif measured and behind == measured:
                    conflicts[i] += 1
    return support, conflicts
