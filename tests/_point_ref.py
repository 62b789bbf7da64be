"""Numpy restatement of the point-set functions of csrc/mp_point.hip: fps, radius,
radius_graph and PointConv's per-edge feature matrix (include/mi355_mp.h "Point
sets").  Everything is float32 elementwise arithmetic, which numpy rounds
operation by operation exactly as the kernels do (they are compiled without
contraction), so the GPU tests compare indices and features for equality.

Squared distance, left to right:
    acc = (a_0 - b_0) * (a_0 - b_0);  acc = acc + (a_d - b_d) * (a_d - b_d), d = 1..D-1
"""
import math

import numpy as np

F32 = np.float32


def _rows(p):
    p = np.asarray(p, dtype=F32)
    return p.reshape(-1, 1) if p.ndim == 1 else p


def d2(a, b):
    """float32 [n]: the squared distance of every row of a [n, D] to the point b [D]."""
    a, b = _rows(a), np.asarray(b, dtype=F32).reshape(-1)
    t = a[:, 0] - b[0]
    acc = t * t
    for d in range(1, a.shape[1]):
        t = a[:, d] - b[d]
        acc = acc + t * t
    assert acc.dtype == F32
    return acc


def sizes_of(batch, n):
    """(starts [G + 1], G) of a sorted batch vector (None: one graph of n)."""
    if batch is None:
        return np.asarray([0, n], dtype=np.int64), 1
    batch = np.asarray(batch, dtype=np.int64)
    assert batch.shape == (n,) and (np.diff(batch) >= 0).all() and (n == 0 or batch[0] >= 0)
    G = int(batch[-1]) + 1 if n else 0
    return np.searchsorted(batch, np.arange(G + 1)).astype(np.int64), G


def keep_count(ratio, n_g):
    """k_g = ceil(fl32(fl32(ratio) * fl32(n_g))), at most n_g: TopKPooling's count."""
    if n_g <= 0:
        return 0
    return max(0, min(int(n_g), int(math.ceil(float(F32(ratio) * F32(n_g))))))


def fps_graph(pos, k, first=0):
    """The k selections (local indices) of one graph, starting at `first`."""
    pos = _rows(pos)
    n = pos.shape[0]
    assert 0 <= first < n
    m = np.full(n, np.inf, dtype=F32)
    out = [int(first)]
    for _ in range(1, k):
        d = d2(pos, pos[out[-1]])
        m = np.where(d < m, d, m)
        out.append(int(np.argmax(m)))                      # the first of equal maxima
    return out[:k]


def fps(pos, batch=None, ratio=0.5, start=None):
    """int64 [K]: grouped by graph, in selection order; start: per-graph offsets or None (0)."""
    pos = _rows(pos)
    starts, G = sizes_of(batch, pos.shape[0])
    out = []
    for g in range(G):
        s0, s1 = int(starts[g]), int(starts[g + 1])
        k = keep_count(ratio, s1 - s0)
        if k:
            first = 0 if start is None else int(start[g])
            out.extend(s0 + i for i in fps_graph(pos[s0:s1], k, first))
    return np.asarray(out, dtype=np.int64)


def radius(x, y, r, batch_x=None, batch_y=None, max_num_neighbors=32):
    """int64 [2, E]: (y index, x index) sorted by y then x; the first max_num_neighbors
    x of the same graph, ascending, with d2(x_i, y) <= fl32(fl32(r) * fl32(r))."""
    x, y = _rows(x), _rows(y)
    assert x.shape[1] == y.shape[1] and max_num_neighbors >= 1
    r2 = F32(r) * F32(r)
    assert r2.dtype == F32
    sx, Gx = sizes_of(batch_x, x.shape[0])
    by = np.zeros(y.shape[0], dtype=np.int64) if batch_y is None else np.asarray(batch_y, dtype=np.int64)
    rows, cols = [], []
    for j in range(y.shape[0]):
        g = int(by[j])
        if not 0 <= g < Gx:
            continue
        c0, c1 = int(sx[g]), int(sx[g + 1])
        if c0 == c1:
            continue
        hits = c0 + np.nonzero(d2(x[c0:c1], y[j]) <= r2)[0][:max_num_neighbors]
        rows.extend([j] * len(hits))
        cols.extend(hits.tolist())
    return np.asarray([rows, cols], dtype=np.int64).reshape(2, -1)


def radius_graph(x, r, batch=None, loop=False, max_num_neighbors=32, flow="source_to_target"):
    """Upstream's recipe over radius(), quirk included: without loops the search keeps
    max_num_neighbors + 1 hits and drops row == col afterwards."""
    row, col = radius(x, x, r, batch, batch, max_num_neighbors if loop else max_num_neighbors + 1)
    if flow == "source_to_target":
        row, col = col, row
    if not loop:
        keep = row != col
        row, col = row[keep], col[keep]
    return np.stack([row, col])


def edge_features(x_src, pos_src, pos_dst, src, dst):
    """float32 [E, F + D]: [x_src[src] | pos_src[src] - pos_dst[dst]] (x_src None: F = 0)."""
    pos_src, pos_dst = _rows(pos_src), _rows(pos_dst)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    rel = pos_src[src] - pos_dst[dst]
    if x_src is None:
        return rel
    return np.concatenate([np.asarray(x_src, dtype=F32)[src], rel], axis=1)
