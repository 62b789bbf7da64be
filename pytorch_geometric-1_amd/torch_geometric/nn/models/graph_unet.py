"""GraphUNet (PyG 1.4.3 nn.models.graph_unet [U], "Graph U-Nets"): an encoder of
GCNConv(improved=True) and TopKPooling steps, a decoder that puts the pooled
nodes back and convolves on the stored graphs.  Before each pooling step the
connectivity is rebuilt as (A + I)^2 without its diagonal: augment_adj, here one
native sparse product with the diagonal dropped as it is written
(mi355_mp.ops.spgemm, csrc/mp_spgemm.hip)."""
import torch
import torch.nn.functional as F

from mi355_mp import ops as _ops

from ..conv import GCNConv
from ..pool import TopKPooling
from ...utils import add_self_loops
from ...utils.repeat import repeat


class GraphUNet(torch.nn.Module):
    def __init__(self, in_channels, hidden_channels, out_channels, depth, pool_ratios=0.5, sum_res=True, act=F.relu):
        super(GraphUNet, self).__init__()
        assert depth >= 1
        self.in_channels, self.hidden_channels, self.out_channels = in_channels, hidden_channels, out_channels
        self.depth = depth
        self.pool_ratios = repeat(pool_ratios, depth)
        self.act = act
        self.sum_res = sum_res
        channels = hidden_channels
        self.down_convs = torch.nn.ModuleList([GCNConv(in_channels, channels, improved=True)])
        self.pools = torch.nn.ModuleList()
        for i in range(depth):
            self.pools.append(TopKPooling(channels, self.pool_ratios[i]))
            self.down_convs.append(GCNConv(channels, channels, improved=True))
        up_in = channels if sum_res else 2 * channels
        self.up_convs = torch.nn.ModuleList([GCNConv(up_in, channels, improved=True) for _ in range(depth - 1)])
        self.up_convs.append(GCNConv(up_in, out_channels, improved=True))
        self.reset_parameters()

    def reset_parameters(self):
        for m in list(self.down_convs) + list(self.pools) + list(self.up_convs):
            m.reset_parameters()

    def forward(self, x, edge_index, batch=None):
        if batch is None:
            batch = edge_index.new_zeros(x.size(0))
        edge_weight = x.new_ones(edge_index.size(1))
        x = self.act(self.down_convs[0](x, edge_index, edge_weight))
        xs, graphs, perms = [x], [(edge_index, edge_weight)], []
        for i in range(1, self.depth + 1):
            edge_index, edge_weight = self.augment_adj(edge_index, edge_weight, x.size(0))
            x, edge_index, edge_weight, batch, perm, _ = self.pools[i - 1](x, edge_index, edge_weight, batch)
            x = self.act(self.down_convs[i](x, edge_index, edge_weight))
            if i < self.depth:
                xs.append(x)
                graphs.append((edge_index, edge_weight))
            perms.append(perm)
        for i in range(self.depth):
            j = self.depth - 1 - i
            res, (edge_index, edge_weight) = xs[j], graphs[j]
            up = torch.zeros_like(res).index_copy(0, perms[j], x)   # perm holds distinct nodes
            x = res + up if self.sum_res else torch.cat((res, up), dim=-1)
            x = self.up_convs[i](x, edge_index, edge_weight)
            if i < self.depth - 1:
                x = self.act(x)
        return x

    def augment_adj(self, edge_index, edge_weight, num_nodes):
        """(A + I)^2 without its diagonal, coalesced and in row-major order: upstream's
        add_self_loops -> sort_edge_index -> spspmm -> remove_self_loops.  The
        weights descend from ones, so the product takes them detached."""
        edge_index, edge_weight = add_self_loops(edge_index, edge_weight, num_nodes=num_nodes)
        w = edge_weight.detach()
        return _ops.spgemm(edge_index, w, edge_index, w, num_nodes, num_nodes, num_nodes, drop_diagonal=True)

    def __repr__(self):
        return "{}({}, {}, {}, depth={}, pool_ratios={})".format(self.__class__.__name__, self.in_channels,
                                                                 self.hidden_channels, self.out_channels, self.depth,
                                                                 self.pool_ratios)
