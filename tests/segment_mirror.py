"""numpy float32 restatement of the contract of include/rgbid_segment.h, written from the contract: points, edges, order, the
sequential union-find loop (`segment_sequential`), an independent restatement of the reservation rounds with a settable window
(`segment_rounds`), labels, histograms, entropy, the negentropy image, the mask levels in closed form (`mask_levels`) and as a literal
replay of the reference's nested loops (`mask_levels_replay`), and the keypoint bits."""
import numpy as np

from tests.test_cpu_cloud import kinv_numpy

F = np.float32
THRESHOLDS = np.array([0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9], F)
NB = ((1, 0), (0, 1), (1, -1), (1, 1))


def split(block, rows, cols):
    N = rows * cols
    b = np.ascontiguousarray(block, np.uint8)
    return b[4 * N:8 * N].view("<f4").copy(), b[8 * N:20 * N].view("<f4").reshape(3, N).copy()


def points(block, rows, cols, K):
    """-> valid [N] bool, pos float32 [N, 3], normals float32 [N, 3]"""
    iD, nrm = split(block, rows, cols)
    N = rows * cols
    with np.errstate(all="ignore"):
        d = F(1.0) / iD
        valid = ~np.isnan(d) & ~np.isnan(nrm[0])
        p = np.arange(N)
        x = (p % cols).astype(np.float64); y = (p // cols).astype(np.float64); one = np.ones(N)
        dd = d.astype(np.float64)
        Ki = kinv_numpy(K)
        Xc = [((dd * Ki[i, 0]) * x + (dd * Ki[i, 1]) * y) + (dd * Ki[i, 2]) * one for i in range(3)]
        I = np.eye(3)
        Xw = [((I[i, 0] * Xc[0] + I[i, 1] * Xc[1]) + I[i, 2] * Xc[2]) + 0.0 for i in range(3)]
    return valid, np.stack(Xw, 1).astype(F), np.ascontiguousarray(nrm.T)


def edges(valid, pos, nrm, rows, cols):
    """-> (ids, a, b, w) of the kept edges in order: ascending weight (-0 == +0), ties by ascending id"""
    N = rows * cols
    pix = np.arange(N); x = pix % cols; y = pix // cols
    ids, ea, eb, ew = [], [], [], []
    with np.errstate(all="ignore"):
        for nb, (ox, oy) in enumerate(NB):
            x2, y2 = x + ox, y + oy
            ok = valid & (x2 < cols) & (y2 >= 0) & (y2 < rows)
            j = np.where(ok, y2 * cols + x2, 0)
            ok &= valid[j]
            i1, i2 = pix[ok], j[ok]
            p1, p2, n1, n2 = pos[i1], pos[i2], nrm[i1], nrm[i2]
            dp = p2 - p1
            norm = np.sqrt((dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1]) + dp[:, 2] * dp[:, 2])
            dot = (n1[:, 0] * n2[:, 0] + n1[:, 1] * n2[:, 1]) + n1[:, 2] * n2[:, 2]
            dot2 = (F(1.0) / norm) * ((n2[:, 0] * dp[:, 0] + n2[:, 1] * dp[:, 1]) + n2[:, 2] * dp[:, 2])
            c = F(1.0) - dot
            c = np.where(dot2 > 0, c * c, c).astype(F)
            keep = ~np.isnan(c)
            ids.append(4 * i1[keep] + nb); ea.append(i1[keep]); eb.append(i2[keep]); ew.append(c[keep])
    ids = np.concatenate(ids); ea = np.concatenate(ea); eb = np.concatenate(eb); ew = np.concatenate(ew).astype(F)
    ew = np.where(ew == 0, F(0.0), ew)                # -0 -> +0: equal in every comparison and sum the loop makes
    o = np.lexsort((ids, ew))
    return ids[o], ea[o], eb[o], ew[o]


def _find(par, x):
    while par[x] != x:
        par[x] = par[par[x]]
        x = par[x]
    return x


def segment_sequential(N, ea, eb, ew, kth, min_size):
    """the sequential loop, union by rank as the reference's graph does -> (root [N], size, th after pass 1 keyed by component members)"""
    kth = F(kth)
    par = list(range(N)); rank = [0] * N; size = [1] * N; th = [kth] * N

    def join(a, b):
        if rank[a] > rank[b]:
            a, b = b, a
        par[a] = b; size[b] += size[a]
        if rank[a] == rank[b]:
            rank[b] += 1
        return b
    for a0, b0, w in zip(ea.tolist(), eb.tolist(), ew):
        a, b = _find(par, a0), _find(par, b0)
        if a != b and w <= th[a] and w <= th[b]:
            r = join(a, b)
            th[r] = F(w + kth / F(size[r]))
    root1 = np.array([_find(par, i) for i in range(N)])
    th1 = np.array([th[r] for r in root1], F)
    size1 = np.array([size[r] for r in root1])
    for a0, b0 in zip(ea.tolist(), eb.tolist()):
        a, b = _find(par, a0), _find(par, b0)
        if a != b and (size[a] < min_size or size[b] < min_size):
            join(a, b)
    root = np.array([_find(par, i) for i in range(N)])
    return dict(root=root, size=np.array([size[r] for r in root]), root1=root1, size1=size1, th1=th1)


def segment_rounds(N, ea, eb, ew, kth, min_size, window):
    """the reservation rounds: the window is the first `window` undecided edges; an edge of equal roots is dropped; every other one
    reserves both roots with the minimum of the positions; the holders of both reservations are decided.  -> as segment_sequential, and
    the rounds of each pass"""
    kth = F(kth)
    par = list(range(N)); size = [1] * N; th = [kth] * N
    E = len(ea); a_l, b_l = ea.tolist(), eb.tolist()
    rounds = []
    snap = None
    for p in (1, 2):
        queue, nxt, r = [], 0, 0
        while True:
            take = min(window - len(queue), E - nxt)
            queue += range(nxt, nxt + take); nxt += take
            if not queue:
                break
            r += 1
            assert r <= E, "a pass ends within E rounds"
            resv, roots = {}, {}
            for pos in queue:
                a, b = _find(par, a_l[pos]), _find(par, b_l[pos])
                roots[pos] = (a, b)
                if a != b:
                    resv[a] = min(resv.get(a, pos), pos); resv[b] = min(resv.get(b, pos), pos)
            stay, merges = [], []
            for pos in queue:
                a, b = roots[pos]
                if a == b:
                    continue
                if resv[a] == pos and resv[b] == pos:
                    w = ew[pos]
                    if (w <= th[a] and w <= th[b]) if p == 1 else (size[a] < min_size or size[b] < min_size):
                        merges.append((a, b, w))
                else:
                    stay.append(pos)
            for a, b, w in merges:          # all at once: the winners own disjoint roots
                lo, hi = min(a, b), max(a, b)
                par[hi] = lo; size[lo] = size[a] + size[b]
                if p == 1:
                    th[lo] = F(w + kth / F(size[lo]))
            queue = stay
        rounds.append(r)
        if p == 1:
            root1 = np.array([_find(par, i) for i in range(N)])
            snap = (root1, np.array([size[x] for x in root1]), np.array([th[x] for x in root1], F))
    root = np.array([_find(par, i) for i in range(N)])
    return dict(root=root, size=np.array([size[r] for r in root]), root1=snap[0], size1=snap[1], th1=snap[2], rounds=tuple(rounds))


def canonical(root, valid):
    """labels by first appearance in raster order (-1 where invalid) and the segment count"""
    lab = np.full(len(root), -1, np.int32)
    seen = {}
    for i in np.nonzero(valid)[0]:
        lab[i] = seen.setdefault(int(root[i]), len(seen))
    return lab, len(seen)


def bins_numpy(nbins):
    i = np.arange(nbins).astype(F)
    inc = F(3.141592) * (F(3.0) - np.sqrt(F(5.0)))
    off = F(2.0) / F(nbins)
    y = (i * off - F(1.0)) + off / F(2.0)
    r = np.sqrt(F(1.0) - y * y)
    phi = i * inc
    return np.stack([np.cos(phi) * r, y, np.sin(phi) * r], 1).astype(F)


def histograms(lab, count, nrm, centres):
    """-> sizes [count], hist [count, nbins] int32, entropy [count] float32"""
    nb = len(centres)
    with np.errstate(all="ignore"):
        d = (nrm[:, 0:1] * centres[None, :, 0] + nrm[:, 1:2] * centres[None, :, 1]) + nrm[:, 2:3] * centres[None, :, 2]
        best = np.full(len(nrm), F(-1.1)); bin_ = np.full(len(nrm), -1)
        for j in range(nb):
            m = d[:, j] > best
            best[m] = d[m, j]; bin_[m] = j
    sizes = np.bincount(lab[lab >= 0], minlength=count).astype(np.int32)
    hist = np.zeros((count, nb), np.int32)
    ok = (lab >= 0) & (bin_ >= 0)
    np.add.at(hist, (lab[ok], bin_[ok]), 1)
    ent = np.zeros(count, F)
    with np.errstate(all="ignore"):
        for s in range(count):
            fs = F(sizes[s]); small = F(1.0) / F(2 * int(sizes[s]))
            acc = F(0.0)
            for j in range(nb):
                freq = F(hist[s, j]) / fs
                acc = F(acc + (F(0.0) if freq < small else F(-freq * np.log(freq))))
            ent[s] = acc / np.log(fs)
    return sizes, hist, ent


def negentropy_image(lab, ent):
    with np.errstate(all="ignore"):
        return np.where(lab >= 0, F(1.0) - ent[np.maximum(lab, 0)] if len(ent) else F(0.0), F(0.0)).astype(F)


def mask_levels(neg, M=4):
    """closed form: k*(m) = the largest k with (float) c_k / (float) pixels < (float) m / (float) M, -1 when none; entry 0 is -1"""
    flat = neg.reshape(-1)
    with np.errstate(invalid="ignore"):
        c = [int((flat < t).sum()) for t in THRESHOLDS]
    out = np.full(M, -1, np.int32)
    for m in range(1, M):
        for k in range(len(THRESHOLDS)):
            if F(c[k]) / F(flat.size) < F(m) / F(M):
                out[m] = k
    return out


def masks_from_levels(neg, levels):
    """[M, ...] bool: mask m keeps a pixel unless negentropy < t_k*(m)"""
    with np.errstate(invalid="ignore"):
        return np.stack([np.ones(neg.shape, bool) if k < 0 else ~(neg < THRESHOLDS[k]) for k in levels])


def masks_replay(neg, M=4):
    """the reference's nested loops (Keyframe::computeMaskedDescriptors) -> [M, rows, cols] bool"""
    rows, cols = neg.shape
    run = np.ones((rows, cols), bool)
    out = [run.copy() for _ in range(M)]
    if M < 2:
        return np.stack(out)
    for t in THRESHOLDS:
        valid_count = rows * cols
        for y in range(rows):
            for x in range(cols):
                if neg[y, x] < t:
                    valid_count -= 1
                    run[y, x] = False
        masked_frac = F(rows * cols - valid_count) / F(rows * cols)
        for m in range(1, M):
            if masked_frac < F(m) / F(M):
                out[m] = run.copy()
    return np.stack(out)


def keypoint_bits(neg, levels, xy):
    """one byte per keypoint (x, y): bit m set when mask m keeps its pixel; outside the image only bit 0"""
    rows, cols = neg.shape
    masks = masks_from_levels(neg, levels)
    out = np.zeros(len(xy), np.uint8)
    for i, (x, y) in enumerate(xy):
        b = 1
        if 0 <= x < cols and 0 <= y < rows:
            for m in range(1, len(levels)):
                b |= int(masks[m, y, x]) << m
        out[i] = b
    return out


def run(block, rows, cols, K, kth=0.6, min_size=300, nbins=80, M=4, centres=None, window=None):
    """the whole contract for one keyframe -> dict"""
    valid, pos, nrm = points(block, rows, cols, K)
    ids, ea, eb, ew = edges(valid, pos, nrm, rows, cols)
    N = rows * cols
    seg = segment_sequential(N, ea, eb, ew, kth, min_size) if window is None else segment_rounds(N, ea, eb, ew, kth, min_size, window)
    lab, count = canonical(seg["root"], valid)
    centres = bins_numpy(nbins) if centres is None else centres
    sizes, hist, ent = histograms(lab, count, nrm, centres)
    neg = negentropy_image(lab, ent).reshape(rows, cols)
    return dict(labels=lab.reshape(rows, cols), count=count, sizes=sizes, hist=hist, entropy=ent, negentropy=neg, levels=mask_levels(neg, M),
                edges=len(ids), seg=seg, valid=valid)
