"""Dense-batch layers (PyG 1.4.3 nn.dense): DenseSAGEConv and dense_diff_pool,
each a fused native call (csrc/mp_dense.hip) or, when the adjacency needs a
gradient, the upstream recipe (nn/dense/_dense.py holds the choice)."""
from .dense_sage_conv import DenseSAGEConv
from .diff_pool import dense_diff_pool

__all__ = ["DenseSAGEConv", "dense_diff_pool"]
