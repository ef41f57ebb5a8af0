"""numpy restatement of include/rgbid_bow.h, written from the contract and not from the kernels: the GPU tests compare
the library with it byte for byte.

 vocabulary  branching factor k (2 .. 16), depth L (1 .. 6).  Node 0 is the root (centroid zero).  Nodes are numbered level by level, within a
             level by parent then child index; a node has 0 or 2 .. k consecutive children.  The words are the leaves, a word's number is its
             node number.
 training    over n descriptors in input order, level by level.  A node of depth < L with >= 2 descriptors is seeded: its first descriptor,
             then repeatedly the descriptor with the largest minimum Hamming distance to the seeds so far (lowest input index on a tie), up to
             k seeds or until that distance is 0.  Fewer than 2 seeds: the node stays a leaf.  Else a = assign(seeds) and at most `iters` times
             centroids = update(a), b = assign(centroids), stop if b == a, a = b.  assign: nearest child by (distance, child index).  update:
             bit set iff 2 * ones > members, a child without members keeps its centroid.  The children hold what a assigns them.
 weights     W_w = (uint32) floor(log(N / n_w) * 65536 + 0.5), 0 when n_w is 0 or N.
 transform   descend by the nearest child; distinct words ascending; a_w = c_w W_w, A = sum a_w, v_w = (a_w << 30) // A; A = 0: empty.
 score       sum over common words of min(v_q, v_c).
 shortlist   candidates c <= q - min_separation with S > 0, the T largest by (S descending, c descending)."""
import numpy as np

POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def distances(desc, centroid):
    """Hamming distance of each row of desc [n, 32] uint8 to one centroid [32] -> int32 [n]"""
    return POP[np.bitwise_xor(desc, centroid[None, :])].sum(1, dtype=np.int32)


def bits_of(desc):
    """[n, 32] uint8 -> [n, 256] uint8, bit t = byte t // 8, bit t % 8"""
    return np.unpackbits(desc, axis=1, bitorder="little")


def assign(desc, cents):
    d = np.stack([distances(desc, c) for c in cents], 1)
    return np.argmin(d, 1)           # the first minimum: the lowest child index


def update(bits, a, cents):
    out = [c.copy() for c in cents]
    for j in range(len(cents)):
        mem = bits[a == j]
        if len(mem):
            ones = mem.sum(0, dtype=np.int64)
            out[j] = np.packbits((2 * ones > len(mem)).astype(np.uint8), bitorder="little")
    return out


def split(desc, bits, k, iters):
    """one node: desc [m, 32] in input order -> (centroids [s][32], child of each descriptor [m]) or None when the node stays a leaf"""
    if len(desc) < 2:
        return None
    seeds = [0]
    mind = distances(desc, desc[0])
    while len(seeds) < k:
        far = int(np.argmax(mind))   # the first maximum: the lowest input index
        if mind[far] == 0:
            break
        seeds.append(far)
        mind = np.minimum(mind, distances(desc, desc[far]))
    if len(seeds) < 2:
        return None
    cents = [desc[s].copy() for s in seeds]
    a = assign(desc, cents)
    for _ in range(iters):
        cents = update(bits, a, cents)
        b = assign(desc, cents)
        if np.array_equal(a, b):
            break
        a = b
    return cents, a


def train(desc, k, depth, iters=10):
    """desc [n, 32] uint8 in input order -> (centroids uint8 [nodes, 32], children int32 [nodes, 2] = first child, number of children)"""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    bits = bits_of(desc)
    cents, children = [np.zeros(32, np.uint8)], [[0, 0]]
    level = [(0, np.arange(len(desc)))]
    for _ in range(depth):
        nxt = []
        for node, idx in level:
            r = split(desc[idx], bits[idx], k, iters)
            if r is None:
                continue
            cs, a = r
            first = len(cents)
            children[node] = [first, len(cs)]
            for j, c in enumerate(cs):
                cents.append(c)
                children.append([0, 0])
                nxt.append((first + j, idx[a == j]))
        level = nxt
    return np.stack(cents), np.array(children, np.int32)


def descend(cents, children, desc):
    """-> the word (leaf node number) of each descriptor, int32 [n]"""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    node = np.zeros(len(desc), np.int32)
    while True:
        inner = children[node, 1] > 0
        if not inner.any():
            return node
        for p in np.unique(node[inner]):
            sel = node == p
            first, cnt = children[p]
            node[sel] = first + assign(desc[sel], cents[first:first + cnt])


def weights(words_per_kf, nodes):
    """words_per_kf: the word arrays of the N keyframes -> uint32 [nodes]"""
    N = len(words_per_kf)
    nw = np.zeros(nodes, np.int64)
    for w in words_per_kf:
        nw[np.unique(w)] += 1
    out = np.zeros(nodes, np.uint32)
    ok = (nw > 0) & (nw < N)
    out[ok] = np.floor(np.log(float(N) / nw[ok].astype(np.float64)) * 65536.0 + 0.5).astype(np.uint32)
    return out


def vector(words, W):
    """the words of one keyframe's descriptors, the weight table -> [(word, value)] ascending by word"""
    if len(words) == 0:
        return []
    w, c = np.unique(np.asarray(words), return_counts=True)
    a = [int(ci) * int(W[wi]) for wi, ci in zip(w, c)]
    A = sum(a)
    if A == 0:
        return []
    return [(int(wi), (ai << 30) // A) for wi, ai in zip(w, a)]


def score(vq, vc):
    dq = dict(vq)
    return sum(min(dq[w], v) for w, v in vc if w in dq)


def shortlist(vectors, min_separation, T):
    """-> (candidates int32 [n, T] -1 padded, scores uint64 [n, T] 0 padded)"""
    n = len(vectors)
    cand = np.full((n, T), -1, np.int32); sc = np.zeros((n, T), np.uint64)
    for q in range(n):
        rows = [(score(vectors[q], vectors[c]), c) for c in range(0, q - min_separation + 1)]
        rows = sorted([r for r in rows if r[0] > 0], key=lambda r: (-r[0], -r[1]))[:T]
        for j, (s, c) in enumerate(rows):
            cand[q, j], sc[q, j] = c, s
    return cand, sc
