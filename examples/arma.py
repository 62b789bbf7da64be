"""The network of the reference's examples/arma.py -- "Graph Neural Networks with
Convolutional ARMA Filters": two ARMAConv layers of 3 parallel stacks and 2
recurrent steps with shared weights and dropout 0.25 on the skip connection, 16
hidden channels, a ReLU after the first and no activation inside the second,
dropout 0.5 in front of each, a log-softmax at the end, trained with Adam (lr
0.01, weight decay 5e-4) -- on the Cora-shaped synthetic graph of
mi355_mp.graphgen.cora_like with its 140 / 500 / 1000 split (the Planetoid
download is not available offline).  Both layers take the fused step of
csrc/mp_arma.hip: (K, C) = (3, 16) and (3, classes).

    PYTHONPATH=pytorch_geometric-1_amd python examples/arma.py [--epochs 400]
"""
import argparse
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch_geometric.nn import ARMAConv  # noqa: E402
from mi355_mp.graphgen import cora_like  # noqa: E402

HIDDEN, STACKS, STEPS, SKIP_DROPOUT = 16, 3, 2, 0.25


class Net(torch.nn.Module):
    def __init__(self, in_channels, out_channels):
        super(Net, self).__init__()
        stacks = dict(num_stacks=STACKS, num_layers=STEPS, shared_weights=True, dropout=SKIP_DROPOUT)
        self.hidden = ARMAConv(in_channels, HIDDEN, **stacks)            # ReLU inside every step (the default)
        self.out = ARMAConv(HIDDEN, out_channels, act=None, **stacks)    # linear steps: the logits

    def forward(self, x, edge_index):
        h = F.dropout(x, p=0.5, training=self.training)
        h = F.relu(self.hidden(h, edge_index))
        h = F.dropout(h, p=0.5, training=self.training)
        return torch.log_softmax(self.out(h, edge_index), dim=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=400)
    args = ap.parse_args(argv)
    torch.manual_seed(0)
    device = torch.device("cuda:0")
    d = cora_like()
    x, edge_index, y = d["x"].to(device), d["edge_index"].to(device), d["y"].to(device)
    splits = [d[k].to(device) for k in ("train_mask", "val_mask", "test_mask")]
    model = Net(x.shape[1], int(y.max()) + 1).to(device)
    assert all(conv.fused(x.new_empty(1, conv.in_channels)) for conv in (model.hidden, model.out))
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
