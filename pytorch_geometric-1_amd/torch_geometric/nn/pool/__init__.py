"""Graph pooling (PyG 1.4.3 nn.pool): TopKPooling on the native engine."""
from .topk_pool import TopKPooling, filter_adj, topk

__all__ = ["TopKPooling", "topk", "filter_adj"]
