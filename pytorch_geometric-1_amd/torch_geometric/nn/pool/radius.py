"""radius and radius_graph (PyG 1.4.3 nn.radius / nn.radius_graph over torch_cluster
1.5 [U]) on the native engine (csrc/mp_point.hip).

For every point of y: the first max_num_neighbors points of x, in ascending
index, that lie in the same graph within distance r.  Upstream leaves which
neighbours survive the cap to the hardware; here it is the ones of lowest index,
and the test is d2(x_i, y) <= fl32(fl32(r) * fl32(r)) on fp32 squared distances
(include/mi355_mp.h "Point sets"): one rounding fewer than sqrt(d2) <= r, exact on
lattice points, the boundary included.  The search is brute force inside each
graph.  There is no CPU path.
"""
import torch

from mi355_mp import _lib, ops


def radius(x, y, r, batch_x=None, batch_y=None, max_num_neighbors=32):
    r"""int64 [2, E]: row 0 indices into y, row 1 indices into x, sorted by y
    then x.

    x [N, D], y [M, D]: float32, D <= 8.  Graph g of batch_y searches graph g of
    batch_x; either may be empty on one side.  ValueError before any search for
    an unsorted batch vector, r negative or not finite, max_num_neighbors < 1,
    x and y of different width.

    Host synchronisation: one device-to-host read (E), beyond the batch layouts,
    which are read once per batch tensor and cached.
    """
    _lib.require_device(x, y, batch_x, batch_y)
    return ops.radius_search(x, y, r, batch_x, batch_y, max_num_neighbors)


def radius_graph(x, r, batch=None, loop=False, max_num_neighbors=32, flow="source_to_target"):
    r"""edge_index int64 [2, E] linking every point to the points within r, by
    upstream's recipe: radius(x, x, r, batch, batch, max_num_neighbors + 1 without
    loops, max_num_neighbors with), the rows swapped for flow='source_to_target',
    and row == col dropped unless `loop`.  As upstream, a node ends with
    max_num_neighbors + 1 neighbours when its own index is not among its first
    max_num_neighbors + 1 hits."""
    assert flow in ["source_to_target", "target_to_source"]
    row, col = radius(x, x, r, batch, batch, max_num_neighbors if loop else max_num_neighbors + 1)
    if flow == "source_to_target":
        row, col = col, row
    if not loop:
        mask = row != col
        row, col = row[mask], col[mask]
    return torch.stack([row, col], dim=0)
