"""PointNet++ segmentation on synthetic clouds: two set abstraction stages (farthest
point sampling, a radius search, PointConv -- the stages of examples/pointnet++.py),
then two feature propagation stages back up to every point -- knn_interpolate with
k = 3 from the coarser level, concatenated with the finer level's own features (the
skip), and an MLP -- and a per-point classifier.  The clouds have the shape
examples/pointnet++.py draws: `--points` points in [-1, 1]^3 around four blobs; a
point's label is the blob it was drawn from, and every cloud is shifted a little,
so a point is labelled from its place in the cloud rather than in space.  Sampling,
both searches, PointConv's edge features and the interpolation are the engine's
kernels.

    PYTHONPATH=pytorch_geometric-1_amd python examples/point_segmentation.py [--epochs 3]
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
from torch_geometric.nn import PointConv, fps, knn_interpolate, radius  # noqa: E402

POINTS = 1024
PARTS = 4


def synthetic_clouds(n_clouds, seed, points=POINTS):
    """n_clouds clouds of `points` points: a mixture of four blobs at fixed centres in
    [-1, 1]^3, the whole cloud shifted by up to 0.2 and clipped to the cube; y [points]:
    the blob of every point."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.rand(PARTS, 3, generator=torch.Generator().manual_seed(1234)) * 1.2 - 0.6
    out = []
    for _ in range(n_clouds):
        blob = torch.randint(PARTS, (points,), generator=g)
        shift = torch.rand(1, 3, generator=g) * 0.4 - 0.2
        pos = centres[blob] + shift + 0.15 * torch.randn(points, 3, generator=g)
        out.append(Data(pos=pos.clamp_(-1, 1), y=blob))
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
        x = self.conv(x, (pos, centre), found.flip(0))  # (point, centre): messages flow to the sample
        return F.relu(x), centre, centre_batch


class FeaturePropagation(torch.nn.Module):
    """Interpolate the coarse level's features onto the fine level's points from their
    3 nearest coarse points, concatenate the fine level's own features, run an MLP."""

    def __init__(self, nn, k=3):
        super(FeaturePropagation, self).__init__()
        self.nn, self.k = nn, k

    def forward(self, x, pos, batch, x_skip, pos_skip, batch_skip):
        x = knn_interpolate(x, pos, pos_skip, batch, batch_skip, k=self.k)
        return F.relu(self.nn(torch.cat([x, x_skip], dim=1)))


class Net(torch.nn.Module):
    def __init__(self):
        super(Net, self).__init__()
        self.sa1 = SetAbstraction(0.5, 0.2, mlp(3, 32, 64))
        self.sa2 = SetAbstraction(0.25, 0.4, mlp(64 + 3, 64, 128))
        self.fp2 = FeaturePropagation(mlp(128 + 64, 128))
        self.fp1 = FeaturePropagation(mlp(128 + 3, 128, 64))
        self.lin1 = Linear(64, 64)
        self.lin2 = Linear(64, PARTS)
        self.kept = None                                # points per level of the last forward

    def forward(self, data):
        pos0, batch0 = data.pos, data.batch
        x1, pos1, batch1 = self.sa1(None, pos0, batch0)
        x2, pos2, batch2 = self.sa2(x1, pos1, batch1)
        self.kept = (pos0.size(0), pos1.size(0), pos2.size(0))
        x = self.fp2(x2, pos2, batch2, x1, pos1, batch1)
        x = self.fp1(x, pos1, batch1, pos0, pos0, batch0)   # no input features: the skip is the coordinates
        x = F.dropout(F.relu(self.lin1(x)), p=0.5, training=self.training)
        return F.log_softmax(self.lin2(x), dim=-1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--points", type=int, default=POINTS)
    args = ap.parse_args(argv)
    loader = DataLoader(synthetic_clouds(args.clouds, 7, args.points), batch_size=args.batch_size, shuffle=True)
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    model = Net().to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=0.005)
    losses = []
    for epoch in range(args.epochs):
        model.train()
        correct = total = 0
        for data in loader:
            data = data.to(device)
            optimizer.zero_grad()
            out = model(data)
            loss = F.nll_loss(out, data.y)
            loss.backward()
            optimizer.step()
            losses.append(float(loss.detach()))
            correct += int((out.argmax(dim=1) == data.y).sum())
            total += data.y.numel()
            print("loss {:.4f}".format(losses[-1]))
        print("Epoch: {:02d}, loss {:.4f}, train accuracy {:.3f}".format(epoch + 1, losses[-1], correct / total))
    return losses


if __name__ == "__main__":
    main()
