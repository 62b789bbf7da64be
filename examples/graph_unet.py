"""The node classifier of "Graph U-Nets": GraphUNet(F, 32, classes, depth=3,
pool_ratios=[2000 / N, 0.5]) behind a dropout of 0.92 on the input features, a
log-softmax, trained with Adam (lr 0.01, weight decay 1e-3) -- on the Cora-shaped
synthetic graph of mi355_mp.graphgen.cora_like with its 140 / 500 / 1000 split
(the Planetoid download is not available offline).  Every pooling step squares
the adjacency with the native sparse product of csrc/mp_spgemm.hip.  Upstream
also drops 20% of the edges per step with dropout_adj, which this package does
not have: the example trains on the full edge list.

    PYTHONPATH=pytorch_geometric-1_amd python examples/graph_unet.py [--nodes 2708] [--epochs 200]
"""
import argparse
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch_geometric.nn import GraphUNet  # noqa: E402
from mi355_mp.graphgen import cora_like  # noqa: E402

CORA_NODES = 2708


class Net(torch.nn.Module):
    def __init__(self, in_channels, out_channels, num_nodes):
        super(Net, self).__init__()
        self.unet = GraphUNet(in_channels, 32, out_channels, depth=3, pool_ratios=[2000 / num_nodes, 0.5])

    def forward(self, x, edge_index):
        x = F.dropout(x, p=0.92, training=self.training)
        return torch.log_softmax(self.unet(x, edge_index), dim=1)


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
    model = Net(x.shape[1], int(y.max()) + 1, args.nodes).to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=0.001)
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
