from .message_passing import MessagePassing
from .gcn_conv import GCNConv
from .gat_conv import GATConv
from .sage_conv import SAGEConv
from .graph_conv import GraphConv
from .cheb_conv import ChebConv
from .agnn_conv import AGNNConv
from .sg_conv import SGConv
from .gin_conv import GINConv
from .spline_conv import SplineConv
from .point_conv import PointConv
from .nn_conv import NNConv
from .rgcn_conv import RGCNConv
from .dna_conv import DNAConv
from .edge_conv import EdgeConv, DynamicEdgeConv
from .gmm_conv import GMMConv

__all__ = ["MessagePassing", "GCNConv", "GATConv", "SAGEConv", "GraphConv", "ChebConv", "AGNNConv", "SGConv", "GINConv",
           "SplineConv", "PointConv", "NNConv", "RGCNConv", "DNAConv", "EdgeConv", "DynamicEdgeConv", "GMMConv"]
