"""Numpy restatement of the nearest-neighbour functions of csrc/mp_knn.hip: knn,
knn_graph, nearest and knn_interpolate (include/mi355_mp.h "Nearest neighbours").
Distances are float32 elementwise arithmetic, which numpy rounds operation by
operation exactly as the kernels do (they are compiled without contraction), and
the selection is an ordering of (d2, index) pairs, so the GPU tests compare
indices for equality.

Squared distance, left to right, any width:
    acc = (a_0 - b_0) * (a_0 - b_0);  acc = acc + (a_d - b_d) * (a_d - b_d), d = 1..D-1

knn_interpolate is restated in float64 FROM THE FLOAT32 d2: the weights
1 / max(d2, 1e-16) and both sums in double, so the kernel's fp32 sums are held to a
bound in ulps of the convex combination they compute.
"""
import numpy as np

from tests._point_ref import d2, sizes_of, _rows

F32 = np.float32
CLAMP = F32(1e-16)


def knn_with_d2(x, y, k, batch_x=None, batch_y=None):
    """(pairs int64 [2, E], d2 float32 [E]): for every row j of y the min(k, n_g) rows
    of x of the same graph smallest under (d2(x_i, y_j), i); sorted by y, ascending
    in that key within a y."""
    x, y = _rows(x), _rows(y)
    assert x.shape[1] == y.shape[1] and k >= 1
    sx, Gx = sizes_of(batch_x, x.shape[0])
    by = np.zeros(y.shape[0], dtype=np.int64) if batch_y is None else np.asarray(batch_y, dtype=np.int64)
    rows, cols, dist = [], [], []
    for j in range(y.shape[0]):
        g = int(by[j])
        if not 0 <= g < Gx:
            continue
        c0, c1 = int(sx[g]), int(sx[g + 1])
        if c0 == c1:
            continue
        d = d2(x[c0:c1], y[j])
        i = np.arange(c1 - c0)
        best = np.lexsort((i, d))[:k]
        rows.extend([j] * len(best))
        cols.extend((c0 + best).tolist())
        dist.extend(d[best].tolist())
    return np.asarray([rows, cols], dtype=np.int64).reshape(2, -1), np.asarray(dist, dtype=F32)


def knn(x, y, k, batch_x=None, batch_y=None):
    return knn_with_d2(x, y, k, batch_x, batch_y)[0]


def knn_graph(x, k, batch=None, loop=False, flow="source_to_target"):
    """Upstream's recipe over knn(), quirk included: without loops the search keeps
    k + 1 hits and drops row == col afterwards."""
    row, col = knn(x, x, k if loop else k + 1, batch, batch)
    if flow == "source_to_target":
        row, col = col, row
    if not loop:
        keep = row != col
        row, col = row[keep], col[keep]
    return np.stack([row, col])


def nearest(x, y, batch_x=None, batch_y=None):
    """int64 [n_x]: row 1 of knn(y, x, 1, batch_y, batch_x); ValueError for an x without a y."""
    pairs = knn(y, x, 1, batch_y, batch_x)
    if pairs.shape[1] < _rows(x).shape[0]:
        raise ValueError("an x lies in a graph without a y")
    return pairs[1]


def interpolation_weights(pairs, dist, n_y):
    """float64 [E]: w_t / W_j of every pair, w = 1 / max(d2, 1e-16) from the float32 d2."""
    w = 1.0 / np.maximum(dist.astype(np.float64), np.float64(CLAMP))
    W = np.zeros(n_y, dtype=np.float64)
    np.add.at(W, pairs[0], w)
    return w / W[pairs[0]]


def knn_interpolate(x, pos_x, pos_y, batch_x=None, batch_y=None, k=3):
    """(out float64 [n_y, C], scale float64 [n_y, C], pairs, weights): the
    interpolation, max_t |x[i_t, c]| of every element (what its bound is relative
    to), the pairs and their normalised weights.  A y without neighbours: zeros."""
    x = np.asarray(x, dtype=F32)
    x = x.reshape(-1, 1) if x.ndim == 1 else x
    n_y = _rows(pos_y).shape[0]
    pairs, dist = knn_with_d2(pos_x, pos_y, k, batch_x, batch_y)
    wn = interpolation_weights(pairs, dist, n_y)
    out = np.zeros((n_y, x.shape[1]), dtype=np.float64)
    np.add.at(out, pairs[0], wn[:, None] * x[pairs[1]].astype(np.float64))
    scale = np.zeros_like(out)
    np.maximum.at(scale, pairs[0], np.abs(x[pairs[1]]).astype(np.float64))
    return out, scale, pairs, wn


def knn_interpolate_grad(g, pairs, wn, n_x):
    """(grad float64 [n_x, C], scale, degree): d x[i] = sum_{(j, i)} wn_ji * g[j], the
    largest |g[j, c]| among the pairs of i, and the in-degree of i."""
    g = np.asarray(g, dtype=np.float64)
    grad = np.zeros((n_x, g.shape[1]), dtype=np.float64)
    np.add.at(grad, pairs[1], wn[:, None] * g[pairs[0]])
    scale = np.zeros_like(grad)
    np.maximum.at(scale, pairs[1], np.abs(g[pairs[0]]))
    return grad, scale, np.bincount(pairs[1], minlength=n_x)
