"""The reference's examples/pointnet++.py -- PointNet++ classification: two set
abstraction stages (farthest point sampling at ratios 0.5 and 0.25, a radius
search of 0.1 and 0.2 capped at 64 neighbours, PointConv over the found edges), a
global stage and a three-layer head -- on synthetic clouds of ModelNet10's shape:
1024 points in [-1, 1]^3 per cloud, 10 classes (ModelNet is not downloadable
offline).  The graph is built on the device in every forward: fps, radius and
PointConv's edge features are the engine's kernels.

    PYTHONPATH=pytorch_geometric-1_amd python "examples/pointnet++.py" [--epochs 3]
"""
import argparse
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch.nn import Linear, ReLU, Sequential  # noqa: E402
from torch_geometric.data import Data, DataLoader  # noqa: E402
from torch_geometric.nn import PointConv, fps, radius  # noqa: E402

POINTS = 1024
CLASSES = 10


def synthetic_clouds(n_clouds, seed, points=POINTS):
    """n_clouds clouds of `points` points: each class is a mixture of four blobs at
    class-specific centres in [-1, 1]^3, clipped to the cube, so there is something
    to learn."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.rand(CLASSES, 4, 3, generator=torch.Generator().manual_seed(1234)) * 1.6 - 0.8
    out = []
    for _ in range(n_clouds):
        y = int(torch.randint(CLASSES, (1,), generator=g))
        blob = torch.randint(4, (points,), generator=g)
        pos = centres[y][blob] + 0.15 * torch.randn(points, 3, generator=g)
        out.append(Data(pos=pos.clamp_(-1, 1), y=torch.tensor([y])))
    return out


def mlp(*widths):
    layers = []
    for a, b in zip(widths[:-1], widths[1:]):
        layers += [Linear(a, b), ReLU()]
    return Sequential(*layers[:-1])


class SetAbstraction(torch.nn.Module):
    """Sample ratio * n_g points per cloud, link each to its neighbours within r
    (at most 64, lowest index first) and run PointConv from the points to the sample."""

    def __init__(self, ratio, r, local_nn):
        super(SetAbstraction, self).__init__()
        self.ratio, self.r = ratio, r
        self.conv = PointConv(local_nn)

    def forward(self, x, pos, batch):
        idx = fps(pos, batch, ratio=self.ratio)
        centre, centre_batch = pos[idx], batch[idx]
        found = radius(pos, centre, self.r, batch, centre_batch, max_num_neighbors=64)
        edge_index = found.flip(0)                      # (point, centre): messages flow to the sample
        x = self.conv(x, (pos, centre), edge_index)
        return F.relu(x), centre, centre_batch


class Net(torch.nn.Module):
    def __init__(self):
        super(Net, self).__init__()
        self.sa1 = SetAbstraction(0.5, 0.1, mlp(3, 64, 64, 128))
        self.sa2 = SetAbstraction(0.25, 0.2, mlp(128 + 3, 128, 128, 256))
        self.global_sa = mlp(256 + 3, 256, 512, 1024)
        self.lin1 = Linear(1024, 512)
        self.lin2 = Linear(512, 256)
        self.lin3 = Linear(256, CLASSES)
        self.kept = None                                # points per stage of the last forward

    def forward(self, data):
        x, pos, batch = self.sa1(None, data.pos, data.batch)
        n1 = pos.size(0)
        x, pos, batch = self.sa2(x, pos, batch)
        self.kept = (n1, pos.size(0))
        x = self.global_sa(torch.cat([x, pos], dim=1))
        x = x.view(data.num_graphs, -1, x.size(1)).max(dim=1)[0]    # every cloud keeps the same count
        x = F.dropout(F.relu(self.lin1(x)), p=0.5, training=self.training)
        x = F.dropout(F.relu(self.lin2(x)), p=0.5, training=self.training)
        return F.log_softmax(self.lin3(x), dim=-1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--points", type=int, default=POINTS)
    args = ap.parse_args(argv)
    loader = DataLoader(synthetic_clouds(args.clouds, 7, args.points), batch_size=args.batch_size, shuffle=True)
    device = torch.device("cuda:0")
    model = Net().to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=0.001)
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
