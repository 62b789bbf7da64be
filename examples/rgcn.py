"""The reference's examples/rgcn.py -- the two-layer relational GCN of "Modeling
Relational Data with Graph Convolutional Networks": RGCNConv(num_nodes, 16, R,
num_bases=30) on no node features (x = None: one embedding row per node and
basis), a ReLU, RGCNConv(16, classes, R, num_bases=30) and a log-softmax,
trained with Adam (lr 0.01, weight decay 5e-4) on the labelled nodes -- on a
synthetic entity graph of the MUTAG graph's shape (the Entities datasets are
not downloadable offline): 23 644 nodes, 74 227 (subject, relation, object)
triples over 23 relations with skewed frequencies, each stored with its inverse
(relation + 23): 148 454 edges, 46 relations, 2 classes, 340 labelled nodes of
which 272 train.  A node's label is a function of the relations of its incoming
edges (the sign of a fixed per-relation weight summed over them, against the
median), so the loss can fall.  --nodes scales every count with the graph.

    PYTHONPATH=pytorch_geometric-1_amd python examples/rgcn.py [--nodes 23644] [--epochs 50]
"""
import argparse
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch_geometric.nn import RGCNConv  # noqa: E402

MUTAG_NODES, MUTAG_TRIPLES, MUTAG_LABELLED = 23644, 74227, 340
BASE_RELATIONS = 23
NUM_RELATIONS = 2 * BASE_RELATIONS
NUM_CLASSES = 2


def entity_graph(n_nodes, seed):
    """(edge_index [2, E], edge_type [E], train_idx, train_y, test_idx, test_y) of a
    synthetic knowledge graph: triples with Zipf-distributed relations, then
    their inverses."""
    g = torch.Generator().manual_seed(seed)
    n_triples = max(int(round(n_nodes * MUTAG_TRIPLES / MUTAG_NODES)), 1)
    freq = 1.0 / torch.arange(1, BASE_RELATIONS + 1, dtype=torch.float64)
    rel = torch.multinomial(freq / freq.sum(), n_triples, replacement=True, generator=g)
    sub = torch.randint(0, n_nodes, (n_triples,), generator=g)
    obj = torch.randint(0, n_nodes, (n_triples,), generator=g)
    edge_index = torch.stack([torch.cat([sub, obj]), torch.cat([obj, sub])])
    edge_type = torch.cat([rel, rel + BASE_RELATIONS])
    weight = torch.randn(NUM_RELATIONS, generator=g)
    score = torch.zeros(n_nodes).index_add_(0, edge_index[1], weight[edge_type])
    y = (score > score.median()).long()
    n_labelled = max(int(round(n_nodes * MUTAG_LABELLED / MUTAG_NODES)), 64)
    labelled = torch.randperm(n_nodes, generator=g)[:n_labelled]
    n_train = (4 * n_labelled) // 5
    train_idx, test_idx = labelled[:n_train], labelled[n_train:]
    return edge_index, edge_type, train_idx, y[train_idx], test_idx, y[test_idx]


class Net(torch.nn.Module):
    def __init__(self, n_nodes):
        super(Net, self).__init__()
        self.conv1 = RGCNConv(n_nodes, 16, NUM_RELATIONS, num_bases=30)
        self.conv2 = RGCNConv(16, NUM_CLASSES, NUM_RELATIONS, num_bases=30)

    def forward(self, edge_index, edge_type):
        x = F.relu(self.conv1(None, edge_index, edge_type))
        x = self.conv2(x, edge_index, edge_type)
        return F.log_softmax(x, dim=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=MUTAG_NODES)
    ap.add_argument("--epochs", type=int, default=50)
    args = ap.parse_args(argv)
    torch.manual_seed(0)
    device = torch.device("cuda:0")
    edge_index, edge_type, train_idx, train_y, test_idx, test_y = (t.to(device) for t in entity_graph(args.nodes, 0))
    model = Net(args.nodes).to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=0.0005)
    losses = []
    for epoch in range(1, args.epochs + 1):
        model.train()
        optimizer.zero_grad()
        loss = F.nll_loss(model(edge_index, edge_type)[train_idx], train_y)
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
        model.eval()
        with torch.no_grad():
            pred = model(edge_index, edge_type)[test_idx].max(1)[1]
        acc = float(pred.eq(test_y).sum()) / max(test_y.numel(), 1)
        print("Epoch: {:02d}, loss {:.6f}, Accuracy: {:.4f}".format(epoch, losses[-1], acc))
    return losses


if __name__ == "__main__":
    main()
