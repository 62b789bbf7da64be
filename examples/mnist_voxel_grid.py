"""The reference's examples/mnist_voxel_grid.py -- the cluster-pooling SplineCNN:
three SplineConv(dim=2, kernel_size=5) layers, voxel_grid at 5, 7 and 14 with
max_pool between them and a max_pool_x(size=4) head -- on synthetic
superpixel-sized graphs: 75 nodes with 2-D positions in [0, 28), 1 feature, 10
classes (MNISTSuperpixels is not downloadable offline).

    PYTHONPATH=pytorch_geometric-1_amd python examples/mnist_voxel_grid.py [--epochs 3]
"""
import argparse
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch_geometric.data import DataLoader  # noqa: E402
from torch_geometric.nn import SplineConv, voxel_grid, max_pool, max_pool_x  # noqa: E402
from torch_geometric.transforms import Cartesian  # noqa: E402

from mnist_spline import superpixel_like  # noqa: E402

transform = Cartesian(cat=False)


def superpixel_graphs(n_graphs, seed):
    """superpixel_like graphs with their positions scaled from the unit square to
    [0, 28), the MNIST superpixel range the voxel sizes are written for."""
    out = superpixel_like(n_graphs, seed)
    for data in out:
        data.pos = data.pos * 28
    return out


class Net(torch.nn.Module):
    def __init__(self):
        super(Net, self).__init__()
        self.conv1 = SplineConv(1, 32, dim=2, kernel_size=5)
        self.conv2 = SplineConv(32, 64, dim=2, kernel_size=5)
        self.conv3 = SplineConv(64, 64, dim=2, kernel_size=5)
        self.fc1 = torch.nn.Linear(4 * 64, 128)
        self.fc2 = torch.nn.Linear(128, 10)

    def forward(self, data):
        data.x = F.elu(self.conv1(data.x, data.edge_index, data.edge_attr))
        cluster = voxel_grid(data.pos, data.batch, size=5, start=0, end=28)
        data = max_pool(cluster, data, transform=transform)

        data.x = F.elu(self.conv2(data.x, data.edge_index, data.edge_attr))
        cluster = voxel_grid(data.pos, data.batch, size=7, start=0, end=28)
        data = max_pool(cluster, data, transform=transform)

        data.x = F.elu(self.conv3(data.x, data.edge_index, data.edge_attr))
        cluster = voxel_grid(data.pos, data.batch, size=14, start=0, end=27.99)
        x, _ = max_pool_x(cluster, data.x, data.batch, size=4)

        x = x.view(-1, self.fc1.weight.size(1))
        x = F.elu(self.fc1(x))
        x = F.dropout(x, training=self.training)
        x = self.fc2(x)
        return F.log_softmax(x, dim=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--graphs", type=int, default=2048)
    args = ap.parse_args(argv)
    loader = DataLoader(superpixel_graphs(args.graphs, 7), batch_size=64, shuffle=True)
    device = torch.device("cuda:0")
    model = Net().to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=0.01)
    losses = []
    for epoch in range(args.epochs):
        model.train()
        for data in loader:
            data = data.to(device)
            optimizer.zero_grad()
            loss = F.nll_loss(model(data), data.y)
            loss.backward()
            optimizer.step()
            losses.append(float(loss.detach()))
        print("Epoch: {:02d}, loss {:.4f}".format(epoch + 1, losses[-1]))
    return losses


if __name__ == "__main__":
    main()
