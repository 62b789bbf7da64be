"""The two-propagation network of "Attention-based Graph Neural Network for
Semi-supervised Learning": a Linear to 16 hidden channels with a ReLU, an
AGNNConv whose beta is frozen at 1 (a buffer), an AGNNConv whose beta is learned,
a Linear to the classes and a log-softmax, dropout 0.5 in front of both Linears,
trained with Adam (lr 0.01, weight decay 5e-4) -- on the Cora-shaped synthetic
graph of mi355_mp.graphgen.cora_like with its 140 / 500 / 1000 split (the
Planetoid download is not available offline).  Both propagations take the fused
pass of csrc/mp_agnn.hip at F = 16.

    PYTHONPATH=pytorch_geometric-1_amd python examples/agnn.py [--nodes 2708] [--epochs 200]
"""
import argparse
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch_geometric.nn import AGNNConv  # noqa: E402
from mi355_mp.graphgen import cora_like  # noqa: E402

HIDDEN = 16
CORA_NODES = 2708


class Net(torch.nn.Module):
    def __init__(self, in_channels, out_channels):
        super(Net, self).__init__()
        self.lin1 = torch.nn.Linear(in_channels, HIDDEN)
        self.prop1 = AGNNConv(requires_grad=False)
        self.prop2 = AGNNConv(requires_grad=True)
        self.lin2 = torch.nn.Linear(HIDDEN, out_channels)

    def forward(self, x, edge_index):
        h = F.dropout(x, training=self.training)
        h = F.relu(self.lin1(h))
        h = self.prop1(h, edge_index)
        h = self.prop2(h, edge_index)
        h = F.dropout(h, training=self.training)
        return torch.log_softmax(self.lin2(h), dim=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=CORA_NODES)
    ap.add_argument("--epochs", type=int, default=200)
    args = ap.parse_args(argv)
    torch.manual_seed(0)
    device = torch.device("cuda:0")
    d = cora_like(num_nodes=args.nodes, num_pairs=5278 * args.nodes // CORA_NODES)
    x, edge_index, y = d["x"].to(device), d["edge_index"].to(device), d["y"].to(device)
    splits = [d[k].to(device) for k in ("train_mask", "val_mask", "test_mask")]
    model = Net(x.shape[1], int(y.max()) + 1).to(device)
    assert all(conv._fused_ok(x.new_empty(1, HIDDEN), edge_index) for conv in (model.prop1, model.prop2))
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
        print("Epoch: {:03d}, loss {:.6f}, beta {:.4f}, Train: {:.4f}, Val: {:.4f}, Test: {:.4f}".format(
            epoch, losses[-1], float(model.prop2.beta), train_acc, best_val, test_at_best))
    return losses


if __name__ == "__main__":
    main()
