from mi355_mp import _lib, ops

from .degree import degree
from .num_nodes import maybe_num_nodes


def normalized_cut(edge_index, edge_attr, num_nodes=None):
    """Normalized cut of every edge (PyG 1.4.3 utils.normalized_cut):

        deg = 1 / degree(row, num_nodes, edge_attr.dtype)
        out = edge_attr * (deg[row] + deg[col])

    on the device: the degree, two native row gathers and the product (three
    roundings in edge_attr's dtype: the reciprocal, the sum, the product).  An
    edge end outside [0, num_nodes) raises IndexError (ops.check_row_index: cached
    per edge_index tensor).  There is no CPU path."""
    _lib.require_device(edge_index, edge_attr)
    row, col = edge_index[0], edge_index[1]
    n = maybe_num_nodes(row, num_nodes)
    ops.check_row_index(edge_index, n, "normalized_cut")
    inv = (1 / degree(row, n, edge_attr.dtype)).view(-1, 1)
    return edge_attr * (ops.gather_rows(inv, row) + ops.gather_rows(inv, col)).view(-1)
