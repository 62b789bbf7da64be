"""to_undirected (PyG 1.4.x utils.undirected [U]): both directions of every
edge, sorted by (row, col) and coalesced -- a key sort and a dedupe in torch
ops, on the device the edge list lives on (the link-prediction split calls it on
host tensors before .to(device))."""
import torch

from .num_nodes import maybe_num_nodes


def to_undirected(edge_index, num_nodes=None):
    num_nodes = maybe_num_nodes(edge_index, num_nodes)
    row, col = edge_index
    row, col = torch.cat([row, col], dim=0), torch.cat([col, row], dim=0)
    n = max(int(num_nodes), 1)
    key = torch.unique(row * n + col)           # sorted, distinct
    return torch.stack([torch.div(key, n, rounding_mode="floor"), key % n], dim=0)
