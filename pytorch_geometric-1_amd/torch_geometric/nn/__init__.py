from .conv import MessagePassing, GCNConv, GATConv, SAGEConv, GraphConv, ChebConv, AGNNConv, SGConv, GINConv, SplineConv
from .conv import PointConv, NNConv, RGCNConv, DNAConv, EdgeConv, DynamicEdgeConv, GMMConv
from .glob import global_add_pool, global_mean_pool, global_max_pool, Set2Set, GlobalAttention
from .pool import (TopKPooling, voxel_grid, consecutive_cluster, max_pool, max_pool_x, avg_pool, avg_pool_x, pool_edge,
                   pool_batch, pool_pos, graclus, fps, radius, radius_graph, knn, knn_graph, nearest)
from .unpool import knn_interpolate
from .dense import DenseSAGEConv, dense_diff_pool
from .models import InnerProductDecoder, GAE, VGAE
from .data_parallel import DataParallel
from . import inits  # noqa: F401

__all__ = ["MessagePassing", "GCNConv", "GATConv", "SAGEConv", "GraphConv", "ChebConv", "AGNNConv", "SGConv",
           "GINConv", "SplineConv", "global_add_pool", "global_mean_pool", "global_max_pool", "TopKPooling",
           "voxel_grid", "consecutive_cluster", "max_pool", "max_pool_x", "avg_pool", "avg_pool_x", "pool_edge",
           "pool_batch", "pool_pos", "graclus", "fps", "radius", "radius_graph", "PointConv", "NNConv", "Set2Set",
           "GlobalAttention", "DataParallel", "RGCNConv", "DNAConv", "EdgeConv", "DynamicEdgeConv", "knn", "knn_graph",
           "nearest", "knn_interpolate", "DenseSAGEConv", "dense_diff_pool", "InnerProductDecoder", "GAE", "VGAE",
           "GMMConv"]
