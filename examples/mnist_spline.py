"""The reference's SplineCNN superpixel pattern (examples/mnist_*: Cartesian
pseudo-coordinates, SplineConv(dim=2, kernel_size=5) layers, global mean
pooling, graph classification), on synthetic superpixel-sized graphs: 75 nodes
with 2-D positions, 1 feature, 10 classes (MNISTSuperpixels is not
downloadable offline).  DataListLoader + nn.DataParallel, as
examples/data_parallel.py.

    PYTHONPATH=pytorch_geometric-1_amd python examples/mnist_spline.py [--epochs 3]
"""
import argparse
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch_geometric.data import Data, DataListLoader  # noqa: E402
from torch_geometric.nn import DataParallel, SplineConv, global_mean_pool  # noqa: E402
from torch_geometric.transforms import Cartesian  # noqa: E402


def superpixel_like(n_graphs, seed, nodes=75, neighbours=8):
    """Graphs of `nodes` points in the unit square, each linked to its nearest
    `neighbours` points; the class shifts the intensities and skews them along x."""
    g = torch.Generator().manual_seed(seed)
    transform = Cartesian(cat=False)
    out = []
    for _ in range(n_graphs):
        y = int(torch.randint(0, 10, (1,), generator=g))
        pos = torch.rand(nodes, 2, generator=g)
        x = torch.rand(nodes, 1, generator=g) + 0.1 * y + 0.05 * y * pos[:, :1]
        d = torch.cdist(pos, pos)
        d.fill_diagonal_(float("inf"))
        nbr = d.topk(neighbours, largest=False).indices                   # [nodes, neighbours]
        row = torch.arange(nodes).view(-1, 1).expand_as(nbr).reshape(-1)
        edge_index = torch.stack([nbr.reshape(-1), row])                 # neighbour -> node
        out.append(transform(Data(x=x, pos=pos, edge_index=edge_index, y=torch.tensor([y]))))
    return out


class Net(torch.nn.Module):
    def __init__(self):
        super(Net, self).__init__()
        self.conv1 = SplineConv(1, 32, dim=2, kernel_size=5)
        self.conv2 = SplineConv(32, 64, dim=2, kernel_size=5)
        self.lin1 = torch.nn.Linear(64, 128)
        self.lin2 = torch.nn.Linear(128, 10)

    def forward(self, data):
        x = F.elu(self.conv1(data.x, data.edge_index, data.edge_attr))
        x = F.elu(self.conv2(x, data.edge_index, data.edge_attr))
        x = global_mean_pool(x, data.batch)
        x = F.elu(self.lin1(x))
        return F.log_softmax(self.lin2(x), dim=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--graphs", type=int, default=2048)
    args = ap.parse_args(argv)
    dataset = superpixel_like(args.graphs, 7)
    loader = DataListLoader(dataset, batch_size=64, shuffle=True)
    model = Net()
    print("Let's use", torch.cuda.device_count(), "GPUs!")
    model = DataParallel(model)
    device = torch.device("cuda:0")
    model = model.to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=0.01)
    losses = []
    for _ in range(args.epochs):
        for data_list in loader:
            optimizer.zero_grad()
            output = model(data_list)
            y = torch.cat([data.y for data in data_list]).to(output.device)
            loss = F.nll_loss(output, y)
            loss.backward()
            optimizer.step()
            losses.append(float(loss.detach()))
        print("Outside Model: num graphs: {}, loss {:.4f}".format(output.size(0), losses[-1]))
    return losses


if __name__ == "__main__":
    main()
