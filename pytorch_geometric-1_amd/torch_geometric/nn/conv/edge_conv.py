"""EdgeConv and DynamicEdgeConv (PyG 1.4.3 nn.conv.edge_conv [U]; Wang et al.,
Dynamic Graph CNN for Learning on Point Clouds):

    x'_i = max_{j in N(i)} nn( [x_i | x_j - x_i] )

Both run on the generic MessagePassing path: the gathers of x_i and x_j and the
segmented max are the engine's, the subtraction, the cat and nn are torch.
DynamicEdgeConv builds its graph in feature space with the native knn_graph on
every call.
"""
import torch

from ..inits import reset
from ..pool.knn import knn_graph
from .message_passing import MessagePassing


class EdgeConv(MessagePassing):
    def __init__(self, nn, aggr="max", **kwargs):
        super(EdgeConv, self).__init__(aggr=aggr, **kwargs)
        self.nn = nn
        self.reset_parameters()

    def reset_parameters(self):
        reset(self.nn)

    def forward(self, x, edge_index):
        x = x.unsqueeze(-1) if x.dim() == 1 else x
        return self.propagate(edge_index, x=x)

    def message(self, x_i, x_j):
        return self.nn(torch.cat([x_i, x_j - x_i], dim=1))

    def __repr__(self):
        return "{}(nn={})".format(self.__class__.__name__, self.nn)


class DynamicEdgeConv(EdgeConv):
    def __init__(self, nn, k, aggr="max", **kwargs):
        super(DynamicEdgeConv, self).__init__(nn=nn, aggr=aggr, **kwargs)
        self.k = k

    def forward(self, x, batch=None):
        """The k nearest neighbours of every row of x among the rows of its graph
        (k + 1 <= 64, up to 256 columns), then EdgeConv over those edges."""
        edge_index = knn_graph(x, self.k, batch, loop=False, flow=self.flow)
        return super(DynamicEdgeConv, self).forward(x, edge_index)

    def __repr__(self):
        return "{}(nn={}, k={})".format(self.__class__.__name__, self.nn, self.k)
