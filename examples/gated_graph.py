"""A GGNN node classifier -- "Gated Graph Sequence Neural Networks" (Li et al.):
the input features projected to 64 channels, one GatedGraphConv of 3 recurrent
steps over them (sum aggregation, one GRU cell shared by the steps), a ReLU and
a linear head, dropout 0.5 in front of the projection and of the head, a
log-softmax at the end, trained with Adam (lr 0.01, weight decay 5e-4) -- on
the Cora-shaped synthetic graph of mi355_mp.graphgen.cora_like with its
140 / 500 / 1000 split (the Planetoid download is not available offline).
Every step takes the fused path: the engine's aggregation of the state and the
one-kernel GRU cell of csrc/mp_gru.hip.

    PYTHONPATH=pytorch_geometric-1_amd python examples/gated_graph.py [--epochs 200]
"""
import argparse
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch_geometric.nn import GatedGraphConv  # noqa: E402
from mi355_mp.graphgen import cora_like  # noqa: E402

HIDDEN, STEPS = 64, 3


class Net(torch.nn.Module):
    def __init__(self, in_channels, out_channels):
        super(Net, self).__init__()
        self.proj = torch.nn.Linear(in_channels, HIDDEN)
        self.ggnn = GatedGraphConv(HIDDEN, STEPS)
        self.head = torch.nn.Linear(HIDDEN, out_channels)

    def forward(self, x, edge_index):
        h = self.proj(F.dropout(x, p=0.5, training=self.training))
        h = F.relu(self.ggnn(h, edge_index))
        h = F.dropout(h, p=0.5, training=self.training)
        return torch.log_softmax(self.head(h), dim=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=200)
    args = ap.parse_args(argv)
    torch.manual_seed(0)
    device = torch.device("cuda:0")
    d = cora_like()
    x, edge_index, y = d["x"].to(device), d["edge_index"].to(device), d["y"].to(device)
    splits = [d[k].to(device) for k in ("train_mask", "val_mask", "test_mask")]
    model = Net(x.shape[1], int(y.max()) + 1).to(device)
    assert model.ggnn.fused(x.new_empty(1, HIDDEN))
    optimizer = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=0.0005)
    losses = []
    best_val = test_at_best = 0.0
    for epoch in range(1, args.epochs + 1):
        model.train()
        optimizer.zero_grad()
        loss = F.nll_loss(model(x, edge_index)[splits[0]], y[splits[0]])
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
        model.eval()
        with torch.no_grad():
            pred = model(x, edge_index).max(1)[1]
        train_acc, val_acc, test_acc = (float(pred[m].eq(y[m]).sum()) / max(int(m.sum()), 1) for m in splits)
        if val_acc > best_val:
            best_val, test_at_best = val_acc, test_acc
        print("Epoch: {:03d}, loss {:.6f}, Train: {:.4f}, Val: {:.4f}, Test: {:.4f}".format(
            epoch, losses[-1], train_acc, best_val, test_at_best))
    return losses


if __name__ == "__main__":
    main()
