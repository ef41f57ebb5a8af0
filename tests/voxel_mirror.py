"""Float32 / float64 numpy restatement of the voxel-grid contract (include/rgbid_voxel.h) that the GPU tests
compare the kernels against byte for byte: PCL's VoxelGrid::applyFilter grid formed in float32, a stable sort of the 64-bit cell keys,
centroids summed in float64 in member (input) order."""
import numpy as np

from rgbid import cloud as CL
from rgbid import voxel as VX


class Refused(ValueError):
    """the library returns RGBID_E_INVALID for this input"""


def _fields(points):
    p = np.ascontiguousarray(points).view(CL.POINT_DTYPE).reshape(-1) if not (isinstance(points, np.ndarray) and points.dtype.names) else points
    return p


def form_grid(lo, hi, leaf):
    """the grid from the finite points' box, in float32 as PCL forms it -> inv (float32 [3]), min_b, div_b, largest cell index per axis"""
    inv, min_b, div_b, span_max = [], [], [], []
    for a in range(3):
        i = np.float32(1.0) / np.float32(leaf[a])
        flo, fhi = np.floor(np.float32(lo[a]) * i), np.floor(np.float32(hi[a]) * i)
        if not (-2.0 ** 31 <= flo < 2.0 ** 31 and -2.0 ** 31 <= fhi < 2.0 ** 31):
            raise Refused(f"axis {a}: floor(box * inv) = {flo}, {fhi} outside int32")
        span = fhi - np.float32(int(flo))
        if not span < 2.0 ** 31:
            raise Refused(f"axis {a}: cell index {span} outside int32")
        inv.append(i); min_b.append(int(flo)); div_b.append(int(fhi) - int(flo) + 1); span_max.append(int(span))
    if div_b[0] * div_b[1] * div_b[2] >= 1 << 62:
        raise Refused("2^62 cells or more")
    return np.array(inv, np.float32), min_b, div_b, span_max


def voxel_numpy(points, leaf=0.01, min_points=0, return_plan=False):
    """rgbid_cloud_point records (structured POINT_DTYPE or [M, 32] uint8) -> VOXEL_DTYPE records; with return_plan also
    dict(min_b, div_b, finite, runs, kept, key_bits).  Raises Refused where the library returns RGBID_E_INVALID."""
    leaf = VX.leaf3(leaf)
    p = _fields(points)
    x, y, z = p["x"], p["y"], p["z"]
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    src = np.nonzero(fin)[0]
    plan = dict(min_b=[0, 0, 0], div_b=[0, 0, 0], finite=int(src.size), runs=0, kept=0, key_bits=0)
    if src.size == 0:
        out = np.zeros(0, VX.VOXEL_DTYPE)
        return (out, plan) if return_plan else out
    xyz = [c[src] for c in (x, y, z)]
    inv, min_b, div_b, span_max = form_grid([c.min() for c in xyz], [c.max() for c in xyz], leaf)
    ijk = [(np.floor(xyz[a] * inv[a]) - np.float32(min_b[a])).astype(np.int64) for a in range(3)]
    key = ijk[0] + ijk[1] * div_b[0] + ijk[2] * (div_b[0] * div_b[1])
    order = np.argsort(key, kind="stable")
    sk = key[order]
    heads = np.r_[True, sk[1:] != sk[:-1]]
    R = int(heads.sum())
    vid = np.empty(src.size, np.int64)
    vid[order] = np.cumsum(heads) - 1                 # each finite point's voxel; bincount below walks them in input (= member) order
    cnt = np.bincount(vid, minlength=R)
    s = [np.bincount(vid, weights=c.astype(np.float64), minlength=R) for c in xyz]
    nrm = [p[f][src] for f in ("nx", "ny", "nz")]
    nf = np.isfinite(nrm[0]) & np.isfinite(nrm[1]) & np.isfinite(nrm[2])
    sn = [np.bincount(vid[nf], weights=c[nf].astype(np.float64), minlength=R) for c in nrm]
    has_n = np.bincount(vid[nf], minlength=R) > 0
    col = [np.bincount(vid, weights=p[c][src].astype(np.float64), minlength=R).astype(np.int64) for c in "rgb"]   # exact below 2^53
    novel = np.bincount(vid, weights=(p["flags"][src] & CL.FLAG_NOVEL).astype(np.float64), minlength=R) > 0
    out = np.zeros(R, VX.VOXEL_DTYPE)
    with np.errstate(all="ignore"):
        for f, v in zip("xyz", s):
            out[f] = (v / cnt).astype(np.float32)
        q = (sn[0] * sn[0] + sn[1] * sn[1]) + sn[2] * sn[2]
        ok = has_n & (q != 0)
        ln = np.sqrt(q)
        for f, v in zip(("nx", "ny", "nz"), sn):
            out[f] = np.where(ok, v / ln, np.nan).astype(np.float32)
    out["count"] = cnt
    for f, v in zip("rgb", col):
        out[f] = v // cnt
    out["flags"] = novel.astype(np.uint8)
    keep = cnt >= min_points
    out = out[keep]
    kmax = span_max[0] + span_max[1] * div_b[0] + span_max[2] * div_b[0] * div_b[1]
    plan.update(min_b=min_b, div_b=div_b, runs=R, kept=int(keep.sum()), key_bits=int(kmax + 1).bit_length())
    return (out, plan) if return_plan else out


def voxel_loops(points, leaf=0.01, min_points=0):
    """an independent restatement: one point at a time with numpy float32 scalars for the grid, a dict of members per key, Python
    floats (double) for the sums"""
    leaf = VX.leaf3(leaf)
    p = _fields(points)
    fin = [i for i in range(len(p)) if all(np.isfinite(p[c][i]) for c in "xyz")]
    if not fin:
        return np.zeros(0, VX.VOXEL_DTYPE)
    lo = [min(p[c][i] for i in fin) for c in "xyz"]
    hi = [max(p[c][i] for i in fin) for c in "xyz"]
    inv = [np.float32(1.0) / np.float32(l) for l in leaf]
    min_b = [int(np.floor(np.float32(lo[a]) * inv[a])) for a in range(3)]
    max_b = [int(np.floor(np.float32(hi[a]) * inv[a])) for a in range(3)]
    div = [max_b[a] - min_b[a] + 1 for a in range(3)]
    members = {}
    for i in fin:
        ijk = [int(np.float32(np.floor(np.float32(p[c][i]) * inv[a])) - np.float32(min_b[a])) for a, c in enumerate("xyz")]
        members.setdefault(ijk[0] + ijk[1] * div[0] + ijk[2] * div[0] * div[1], []).append(i)
    rows = []
    for k in sorted(members):
        m = members[k]
        if len(m) < min_points:
            continue
        n = len(m)
        c = [0.0, 0.0, 0.0]; sn = [0.0, 0.0, 0.0]; has = False; rgb = [0, 0, 0]; fl = 0
        for i in m:
            for a, f in enumerate("xyz"):
                c[a] += float(p[f][i])
            nv = [float(p[f][i]) for f in ("nx", "ny", "nz")]
            if all(np.isfinite(nv)):
                has = True
                for a in range(3):
                    sn[a] += nv[a]
            for a, f in enumerate("rgb"):
                rgb[a] += int(p[f][i])
            fl |= int(p["flags"][i]) & 1
        q = (sn[0] * sn[0] + sn[1] * sn[1]) + sn[2] * sn[2]
        nrm = [s / np.sqrt(q) for s in sn] if has and q != 0 else [float("nan")] * 3
        rows.append(tuple(np.float32(v / n) for v in c) + tuple(np.float32(v) for v in nrm) + (n,) + tuple(v // n for v in rgb) + (fl,))
    return np.array(rows, VX.VOXEL_DTYPE)
