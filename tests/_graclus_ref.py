"""CPU restatement of graclus (include/mi355_mp.h "Graclus"), in plain Python and
numpy: the priority of an entry, the serial greedy matching that defines the
result, the round-by-round handshake the kernels run (with its round count), and
normalized_cut in float64.  The GPU tests compare the native layer against these;
tests/test_graclus_host.py pins them by hand values."""
import struct

import numpy as np

M64 = (1 << 64) - 1


# (name, edge_index, weight, n, cluster): answers worked out by hand from the definition
HAND = [
    # the heaviest pair (1, 2) first; (2, 3) and (0, 1) then each have a matched end
    ("weighted path of 4", [[0, 1, 2], [1, 2, 3]], [1.0, 3.0, 2.0], 4, [0, 1, 1, 3]),
    ("triangle", [[0, 1, 2], [1, 2, 0]], [1.0, 2.0, 3.0], 3, [0, 1, 0]),
    # the pair (0, 1) carries 5, its larger entry: it beats (1, 2) at 3, which the entry at 1 alone would not
    ("repeated pair, two weights", [[0, 1, 1], [1, 0, 2]], [1.0, 5.0, 3.0], 3, [0, 0, 2]),
    ("one-direction edges", [[2, 3], [0, 1]], [1.0, 1.0], 4, [0, 1, 0, 1]),
    ("self-loops only", [[0, 1, 1], [0, 1, 1]], [9.0, 9.0, 9.0], 2, [0, 1]),
    ("isolated nodes", [[1], [3]], None, 5, [0, 1, 2, 1, 4]),
    ("a loop does not match, its node's edge does", [[1, 1], [1, 2]], [9.0, -1.0], 3, [0, 1, 1]),
    ("negative weights order below zero", [[0, 1], [1, 2]], [-2.0, -1.0], 3, [0, 1, 1]),
    ("-0.0 < +0.0", [[0, 1], [1, 2]], [0.0, -0.0], 3, [0, 0, 2]),
    ("E = 0", [[], []], None, 3, [0, 1, 2]),
    ("N = 1", [[], []], None, 1, [0]),
    ("N = 0", [[], []], None, 0, []),
]


def mix64(z):
    """The splitmix64 finaliser."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def wkey(w):
    """The order-preserving uint32 image of a float32 weight."""
    u = struct.unpack("<I", struct.pack("<f", w))[0]
    return (u ^ 0xFFFFFFFF) if u >> 31 else (u | 0x80000000)


def pair_hash(seed, a, b):
    return mix64(mix64(seed & M64) ^ ((a << 32) | b)) >> 32


def _lists(edge_index, weight):
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    w = None if weight is None else np.asarray(weight, dtype=np.float32).reshape(-1)
    assert w is None or w.shape[0] == ei.shape[1]
    return ei[0].tolist(), ei[1].tolist(), None if w is None else w.tolist()


def priorities(edge_index, weight=None, seed=0):
    """One (wkey, h, a, b) per entry in edge order; None for a loop."""
    row, col, w = _lists(edge_index, weight)
    out = []
    for e, (u, v) in enumerate(zip(row, col)):
        if u == v:
            out.append(None)
            continue
        a, b = min(u, v), max(u, v)
        out.append((0 if w is None else wkey(w[e]), pair_hash(seed, a, b), a, b))
    return out


def _check(keys, n):
    for k in keys:
        if k is not None and not (0 <= k[2] and k[3] < n):
            raise IndexError("graclus: an edge end lies outside [0, %d)" % n)


def num_nodes(edge_index, n=None):
    if n is not None:
        return int(n)
    ei = np.asarray(edge_index, dtype=np.int64)
    return int(ei.max()) + 1 if ei.size else 0


def greedy(edge_index, weight=None, n=None, seed=0):
    """The definition: walk the entries in descending priority, match a pair whose
    ends are both unmatched.  cluster [n] int64."""
    n = num_nodes(edge_index, n)
    keys = priorities(edge_index, weight, seed)
    row, col, _ = _lists(edge_index, None)
    if any(not (0 <= u < n and 0 <= v < n) for u, v in zip(row, col)):
        raise IndexError("graclus: an edge end lies outside [0, %d)" % n)
    cluster = list(range(n))
    matched = [False] * n
    for k in sorted((k for k in keys if k is not None), reverse=True):
        a, b = k[2], k[3]
        if not matched[a] and not matched[b]:
            matched[a] = matched[b] = True
            cluster[b] = a
    return np.asarray(cluster, dtype=np.int64).reshape(n)


def handshake(edge_index, weight=None, n=None, seed=0):
    """(cluster, rounds) of the parallel form: every live node (it has an entry
    that is no loop, is unmatched, and found a candidate in every round so far)
    points at its best entry among unmatched neighbours; mutual pointers match;
    a node that finds nobody drops out.  A round is counted while somebody is
    live at its start."""
    n = num_nodes(edge_index, n)
    keys = priorities(edge_index, weight, seed)
    _check(keys, n)
    adj = [[] for _ in range(n)]
    for k in keys:
        if k is not None:
            adj[k[2]].append((k, k[3]))
            adj[k[3]].append((k, k[2]))
    cluster = list(range(n))
    matched = [False] * n
    live = set(i for i in range(n) if adj[i])
    rounds = 0
    while live:
        rounds += 1
        ptr = {}
        for u in live:
            cand = [(k, v) for k, v in adj[u] if not matched[v]]
            ptr[u] = max(cand)[1] if cand else -1
        nxt = set()
        for u in live:
            p = ptr[u]
            if p < 0:
                continue
            if ptr.get(p) == u:
                matched[u] = True
                cluster[u] = min(u, p)
            else:
                nxt.add(u)
        live = nxt
    return np.asarray(cluster, dtype=np.int64).reshape(n), rounds


def normalized_cut(edge_index, edge_attr, n=None):
    """edge_attr * (1 / deg[row] + 1 / deg[col]) in float64, deg = the number of
    edges a node starts."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    n = num_nodes(ei[0], n)
    deg = np.bincount(ei[0], minlength=n).astype(np.float64)
    with np.errstate(divide="ignore"):
        inv = 1.0 / deg
    return np.asarray(edge_attr, dtype=np.float64) * (inv[ei[0]] + inv[ei[1]])


def check_matching(cluster, edge_index):
    """The properties of any valid maximal matching, without the restatement."""
    c = np.asarray(cluster, dtype=np.int64)
    n = c.shape[0]
    idx = np.arange(n)
    assert np.array_equal(c[c], c) and bool((c <= idx).all())
    sizes = np.bincount(c, minlength=n)
    assert int(sizes.max(initial=0)) <= 2
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    pairs = set((min(u, v), max(u, v)) for u, v in zip(ei[0].tolist(), ei[1].tolist()) if u != v)
    for i in idx[c != idx].tolist():
        assert (int(c[i]), i) in pairs                       # paired nodes are adjacent
    single = sizes[c] == 1
    for a, b in pairs:
        assert not (single[a] and single[b]), (a, b)         # no edge joins two singletons
