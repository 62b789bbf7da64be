"""train_test_split_edges (PyG 1.4.x [U]): the link-prediction split of a Data
object's undirected edges, in torch ops only, so it runs where the edge list
lives -- the reference's examples/autoencoder.py calls it before .to(device).
The permutations come from torch's generator (upstream draws the negatives with
Python's random.sample).  data.edge_index is left in place: the reference's example
encodes over it after the split (the upstream version it was written for keeps
it; later ones set it to None)."""
import math

import torch

from .undirected import to_undirected


def train_test_split_edges(data, val_ratio=0.05, test_ratio=0.1):
    assert "batch" not in data  # no batch-mode support
    num_nodes = data.num_nodes
    row, col = data.edge_index
    dev = row.device

    # the upper triangular portion
    mask = row < col
    row, col = row[mask], col[mask]
    n_v = int(math.floor(val_ratio * row.size(0)))
    n_t = int(math.floor(test_ratio * row.size(0)))

    # positive edges: val and test directed, train in both directions
    perm = torch.randperm(row.size(0), device=dev)
    row, col = row[perm], col[perm]
    data.val_pos_edge_index = torch.stack([row[:n_v], col[:n_v]], dim=0)
    data.test_pos_edge_index = torch.stack([row[n_v:n_v + n_t], col[n_v:n_v + n_t]], dim=0)
    data.train_pos_edge_index = to_undirected(torch.stack([row[n_v + n_t:], col[n_v + n_t:]], dim=0), num_nodes)

    # negative edges: distinct non-edges of the upper triangle
    neg_adj_mask = torch.ones(num_nodes, num_nodes, dtype=torch.bool, device=dev).triu(diagonal=1)
    neg_adj_mask[row, col] = False
    neg_row, neg_col = neg_adj_mask.nonzero(as_tuple=True)
    perm = torch.randperm(neg_row.size(0), device=dev)[:min(n_v + n_t, neg_row.size(0))]
    neg_row, neg_col = neg_row[perm], neg_col[perm]
    neg_adj_mask[neg_row, neg_col] = False
    data.train_neg_adj_mask = neg_adj_mask
    data.val_neg_edge_index = torch.stack([neg_row[:n_v], neg_col[:n_v]], dim=0)
    data.test_neg_edge_index = torch.stack([neg_row[n_v:n_v + n_t], neg_col[n_v:n_v + n_t]], dim=0)
    return data
