from .num_nodes import maybe_num_nodes
from .scatter import scatter_
from .softmax import softmax
from .loop import (contains_self_loops, remove_self_loops, add_self_loops,
                   add_remaining_self_loops)
from .degree import degree
from .get_laplacian import get_laplacian
from .repeat import repeat
from .normalized_cut import normalized_cut
from .to_dense import to_dense_batch, to_dense_adj
from .undirected import to_undirected
from .negative_sampling import negative_sampling, structured_negative_sampling
from .train_test_split_edges import train_test_split_edges

__all__ = ["maybe_num_nodes", "scatter_", "softmax", "contains_self_loops", "remove_self_loops",
           "add_self_loops", "add_remaining_self_loops", "degree", "get_laplacian", "repeat",
           "normalized_cut", "to_dense_batch", "to_dense_adj", "to_undirected", "negative_sampling",
           "structured_negative_sampling", "train_test_split_edges"]
