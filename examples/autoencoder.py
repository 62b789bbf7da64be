"""The reference's examples/autoencoder.py (GAE / VGAE link prediction on Cora with a
two-layer GCN encoder, cached=True), unchanged in its model and training loop, on
the Cora-shaped synthetic graph (mi355_mp.graphgen.cora_like: the Planetoid
download is not available offline).  split_edges runs on the host tensors, as
in the reference; the decoder, the reconstruction loss and the negative sampler
run on the native link kernels.

    PYTHONPATH=pytorch_geometric-1_amd python examples/autoencoder.py [--model GAE|VGAE] [--epochs 200]
"""
import argparse
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch_geometric.data import Data  # noqa: E402
from torch_geometric.nn import GCNConv, GAE, VGAE  # noqa: E402
from mi355_mp.graphgen import cora_like  # noqa: E402


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--model", type=str, default="GAE")
    parser.add_argument("--epochs", type=int, default=200)
    args = parser.parse_args(argv)
    assert args.model in ["GAE", "VGAE"]
    kwargs = {"GAE": GAE, "VGAE": VGAE}

    torch.manual_seed(0)
    d = cora_like()
    data = Data(x=d["x"], edge_index=d["edge_index"])
    num_features = data.num_features

    class Encoder(torch.nn.Module):
        def __init__(self, in_channels, out_channels):
            super(Encoder, self).__init__()
            self.conv1 = GCNConv(in_channels, 2 * out_channels, cached=True)
            if args.model in ["GAE"]:
                self.conv2 = GCNConv(2 * out_channels, out_channels, cached=True)
            elif args.model in ["VGAE"]:
                self.conv_mu = GCNConv(2 * out_channels, out_channels, cached=True)
                self.conv_logvar = GCNConv(2 * out_channels, out_channels, cached=True)

        def forward(self, x, edge_index):
            x = F.relu(self.conv1(x, edge_index))
            if args.model in ["GAE"]:
                return self.conv2(x, edge_index)
            elif args.model in ["VGAE"]:
                return self.conv_mu(x, edge_index), self.conv_logvar(x, edge_index)

    channels = 16
    device = torch.device("cuda")
    model = kwargs[args.model](Encoder(num_features, channels)).to(device)
    data = model.split_edges(data)
    x, edge_index = data.x.to(device), data.edge_index.to(device)
    train_pos = data.train_pos_edge_index.to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=0.01)

    def train():
        model.train()
        optimizer.zero_grad()
        z = model.encode(x, edge_index)
        loss = model.recon_loss(z, train_pos)
        if args.model in ["VGAE"]:
            loss = loss + 0.001 * model.kl_loss()
        loss.backward()
        optimizer.step()
        return float(loss.detach())

    def test(pos_edge_index, neg_edge_index):
        model.eval()
        with torch.no_grad():
            z = model.encode(x, edge_index)
        return model.test(z, pos_edge_index.to(device), neg_edge_index.to(device))

    losses = []
    for epoch in range(1, args.epochs + 1):
        losses.append(train())
        print("loss %.6f" % losses[-1])
        auc, ap = test(data.val_pos_edge_index, data.val_neg_edge_index)
        print("Epoch: {:03d}, AUC: {:.4f}, AP: {:.4f}".format(epoch, auc, ap))

    auc, ap = test(data.test_pos_edge_index, data.test_neg_edge_index)
    print("Test AUC: {:.4f}, Test AP: {:.4f}".format(auc, ap))
    return losses


if __name__ == "__main__":
    main()
