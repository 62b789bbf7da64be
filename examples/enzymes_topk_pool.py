"""The reference's top-k pooling model (examples/enzymes_topk_pool.py, and
topk_pool_Net of ConvexPruning.py): three times GraphConv(., 128) ->
TopKPooling(128, ratio=0.8) with global max | mean pooling after each stage,
then three linear layers; graph classification with nll_loss.  ENZYMES is not
downloadable offline, so the data is synthetic and ENZYMES-shaped: 600 graphs
of 2-126 nodes, about 62 undirected edges each, 3 node features, 6 classes.
The label is computable from the graph (the dominant feature column and whether
the graph is larger than the median), so the loss can fall.

    PYTHONPATH=pytorch_geometric-1_amd python examples/enzymes_topk_pool.py [--epochs 5]
"""
import argparse
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch_geometric.data import Data, DataLoader  # noqa: E402
from torch_geometric.nn import GraphConv, TopKPooling  # noqa: E402
from torch_geometric.nn import global_max_pool as gmp, global_mean_pool as gap  # noqa: E402

NUM_FEATURES, NUM_CLASSES = 3, 6


def enzymes_like(n_graphs, seed):
    """Graphs of 2..126 nodes (mean about 33) with about 62 undirected edges;
    class = 2 * (dominant feature column) + (more than 30 nodes)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n_graphs):
        n = int(torch.randint(2, 60, (1,), generator=g)) if float(torch.rand(1, generator=g)) < 0.92 \
            else int(torch.randint(60, 127, (1,), generator=g))
        col = int(torch.randint(0, 3, (1,), generator=g))
        x = 0.3 * torch.rand(n, NUM_FEATURES, generator=g)
        x[:, col] += 0.7
        m = max(1, min(62, n * (n - 1) // 2))
        a = torch.randint(0, n, (m,), generator=g)
        b = (a + 1 + torch.randint(0, n - 1, (m,), generator=g)) % n        # no self loops
        edge_index = torch.cat([torch.stack([a, b]), torch.stack([b, a])], dim=1)
        out.append(Data(x=x, edge_index=edge_index, y=torch.tensor([2 * col + int(n > 30)])))
    return out


class Net(torch.nn.Module):
    def __init__(self):
        super(Net, self).__init__()
        self.conv1 = GraphConv(NUM_FEATURES, 128)
        self.pool1 = TopKPooling(128, ratio=0.8)
        self.conv2 = GraphConv(128, 128)
        self.pool2 = TopKPooling(128, ratio=0.8)
        self.conv3 = GraphConv(128, 128)
        self.pool3 = TopKPooling(128, ratio=0.8)
        self.lin1 = torch.nn.Linear(256, 128)
        self.lin2 = torch.nn.Linear(128, 64)
        self.lin3 = torch.nn.Linear(64, NUM_CLASSES)

    def forward(self, data):
        x, edge_index, batch = data.x, data.edge_index, data.batch
        x = F.relu(self.conv1(x, edge_index))
        x, edge_index, _, batch, _, _ = self.pool1(x, edge_index, None, batch)
        x1 = torch.cat([gmp(x, batch), gap(x, batch)], dim=1)
        x = F.relu(self.conv2(x, edge_index))
        x, edge_index, _, batch, _, _ = self.pool2(x, edge_index, None, batch)
        x2 = torch.cat([gmp(x, batch), gap(x, batch)], dim=1)
        x = F.relu(self.conv3(x, edge_index))
        x, edge_index, _, batch, _, _ = self.pool3(x, edge_index, None, batch)
        x3 = torch.cat([gmp(x, batch), gap(x, batch)], dim=1)
        x = x1 + x2 + x3
        x = F.relu(self.lin1(x))
        x = F.dropout(x, p=0.5, training=self.training)
        x = F.relu(self.lin2(x))
        return F.log_softmax(self.lin3(x), dim=-1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=600)
    ap.add_argument("--batch-size", type=int, default=60)
    ap.add_argument("--lr", type=float, default=0.0005)
    args = ap.parse_args(argv)
    dataset = enzymes_like(args.graphs, 11)
    n_test = len(dataset) // 10
    test_loader = DataLoader(dataset[:n_test], batch_size=args.batch_size)
    train_loader = DataLoader(dataset[n_test:], batch_size=args.batch_size)
    device = torch.device("cuda:0")
    model = Net().to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=args.lr)

    def train():
        model.train()
        loss_all = 0.0
        for data in train_loader:
            data = data.to(device)
            optimizer.zero_grad()
            loss = F.nll_loss(model(data), data.y)
            loss.backward()
            loss_all += data.num_graphs * loss.item()
            optimizer.step()
        return loss_all / (len(dataset) - n_test)

    def test(loader):
        model.eval()
        correct, total = 0, 0
        with torch.no_grad():
            for data in loader:
                data = data.to(device)
                correct += int(model(data).max(dim=1)[1].eq(data.y).sum())
                total += data.num_graphs
        return correct / max(total, 1)

    losses = []
    for epoch in range(1, args.epochs + 1):
        losses.append(train())
        print("Epoch: {:03d}, Loss: {:.5f}, Train Acc: {:.5f}, Test Acc: {:.5f}".format(
            epoch, losses[-1], test(train_loader), test(test_loader)))
    return losses


if __name__ == "__main__":
    main()
