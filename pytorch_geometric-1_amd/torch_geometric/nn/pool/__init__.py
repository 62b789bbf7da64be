"""Graph pooling (PyG 1.4.3 nn.pool): TopKPooling and the cluster pools
(voxel_grid, graclus, max_pool, avg_pool) and the point-set samplers and searches
(fps, radius, radius_graph, knn, knn_graph, nearest) on the native engine."""
from .topk_pool import TopKPooling, filter_adj, topk
from .voxel_grid import voxel_grid
from .graclus import graclus
from .consecutive import consecutive_cluster
from .pool import pool_edge, pool_batch, pool_pos
from .max_pool import max_pool, max_pool_x
from .avg_pool import avg_pool, avg_pool_x
from .fps import fps
from .radius import radius, radius_graph
from .knn import knn, knn_graph, nearest

__all__ = ["TopKPooling", "topk", "filter_adj", "voxel_grid", "consecutive_cluster", "pool_edge", "pool_batch",
           "pool_pos", "max_pool", "max_pool_x", "avg_pool", "avg_pool_x", "graclus", "fps", "radius", "radius_graph", "knn",
           "knn_graph", "nearest"]
