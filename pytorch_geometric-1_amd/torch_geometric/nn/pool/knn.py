"""knn, knn_graph and nearest (PyG 1.4.3 nn.knn / nn.knn_graph / nn.nearest over
torch_cluster 1.5 [U]) on the native engine (csrc/mp_knn.hip).

For every point of y: the k points of x of the same graph that are smallest
under the key (d2(x_i, y_j), i), with d2 the fp32 squared distance of
include/mi355_mp.h "Nearest neighbours" (every operation rounded, left to
right).  Upstream leaves the order of equal distances to the hardware; here they
go to the lower index, so the result is a pure function of its inputs
(tests/_knn_ref.py restates it in numpy).  The search is brute force inside each
graph, at most 64 neighbours (one slot per lane of the selecting wave), rows of up
to MP_KNN_MAX_D (256) columns.  There is no CPU path, and cosine=True is not
implemented.
"""
import torch

from mi355_mp import _lib, ops


def _no_cosine(cosine, what):
    if cosine:
        raise NotImplementedError("%s: cosine=True is not implemented (Euclidean distance only)" % what)


def knn(x, y, k, batch_x=None, batch_y=None, cosine=False):
    r"""int64 [2, E]: row 0 indices into y, row 1 indices into x, sorted by y and
    within a y ascending in (distance, index).

    x [N, D], y [M, D]: float32, D <= 256.  Graph g of batch_y searches graph g of
    batch_x; either may be empty on one side, and a graph of fewer than k points
    gives all of them.  ValueError before any search for an unsorted batch vector,
    a batch vector on one side only, k < 1, k > 64 (the limit of the selection:
    one slot per lane), x and y of different width or wider than 256.

    Host synchronisation: at most one device-to-host read (E), beyond the batch
    layouts, which are read once per batch tensor and cached; none when both batch
    vectors are None.
    """
    _no_cosine(cosine, "knn")
    _lib.require_device(x, y, batch_x, batch_y)
    return ops.knn_search(x, y, k, batch_x, batch_y)


def knn_graph(x, k, batch=None, loop=False, flow="source_to_target", cosine=False):
    r"""edge_index int64 [2, E] linking every point to its k nearest, by
    upstream's recipe: knn(x, x, k + 1 without loops, k with, batch, batch), the
    rows swapped for flow='source_to_target', and row == col dropped unless `loop`.
    As upstream, a node ends with k + 1 neighbours when its own index is not among
    its first k + 1 hits: k + 1 or more coincident points of lower index come
    first.  Without loops k + 1 must be at most 64."""
    assert flow in ["source_to_target", "target_to_source"]
    _no_cosine(cosine, "knn_graph")
    row, col = knn(x, x, k if loop else k + 1, batch, batch)
    if flow == "source_to_target":
        row, col = col, row
    if not loop:
        mask = row != col
        row, col = row[mask], col[mask]
    return torch.stack([row, col], dim=0)


def nearest(x, y, batch_x=None, batch_y=None):
    r"""int64 [N]: for every row of x the index of the nearest row of y in the
    same graph, equal distances to the lower index: row 1 of
    knn(y, x, 1, batch_y, batch_x).  ValueError when some x lies in a graph
    without a y."""
    _lib.require_device(x, y, batch_x, batch_y)
    pairs = ops.knn_search(y, x, 1, batch_y, batch_x)
    n = x.shape[0]
    if pairs.shape[1] < n:
        raise ValueError("nearest: %d rows of x lie in a graph that holds no row of y" % (n - pairs.shape[1]))
    return pairs[1]
