"""sort_edge_index (PyG 1.4.3 utils [U]): the edges in row-major order, their
attributes with them -- one stable sort of the key row * N + col, on the device
the edge list lives on."""
import torch

from .num_nodes import maybe_num_nodes


def sort_edge_index(edge_index, edge_attr=None, num_nodes=None):
    num_nodes = maybe_num_nodes(edge_index, num_nodes)
    perm = torch.sort(edge_index[0] * max(int(num_nodes), 1) + edge_index[1], stable=True).indices
    return edge_index[:, perm], (None if edge_attr is None else edge_attr[perm])
