"""The reference's examples/qm9_nn_conv.py -- the MPNN of "Neural Message Passing
for Quantum Chemistry": a Linear embedding, three rounds of NNConv(aggr='mean')
whose edge network maps the 5 edge columns through Linear(5, 128) -> ReLU ->
Linear(128, dim * dim) followed by a GRU cell, a Set2Set(dim, processing_steps=3)
readout and two Linear layers, trained with an MSE loss on one normalised target
-- on synthetic QM9-shaped molecules (QM9 is not downloadable offline): 3 to 29
atoms with 13 node features and 3-D positions, a sparse bond list with 4 one-hot
bond columns, completed to all ordered atom pairs by the example's own Complete
transform, then Distance(norm=False): 5 edge columns.  The target is a smooth
function of the atoms' features and the molecule's size.

    PYTHONPATH=pytorch_geometric-1_amd python examples/qm9_nn_conv.py [--epochs 3]
"""
import argparse
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import torch_geometric.transforms as T  # noqa: E402
from torch.nn import GRU, Linear, ReLU, Sequential  # noqa: E402
from torch_geometric.data import Data, DataLoader  # noqa: E402
from torch_geometric.nn import NNConv, Set2Set  # noqa: E402

dim = 64
NUM_FEATURES = 13


class Complete(object):
    """Turns the bond list into the complete directed graph on the atoms: every
    ordered pair (i, j), i != j, in row-major order.  A pair that was a bond
    keeps its attribute row, every other pair gets a row of zeros."""

    def __call__(self, data):
        n = data.x.size(0)
        i, j = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
        off_diagonal = (i != j).view(-1)
        pairs = torch.stack([i.reshape(-1), j.reshape(-1)])[:, off_diagonal]
        if data.edge_attr is not None:
            bonds = data.edge_attr.view(data.edge_attr.size(0), -1)
            dense = bonds.new_zeros(n * n, bonds.size(1))              # one row per ordered pair, the diagonal included
            dense[data.edge_index[0] * n + data.edge_index[1]] = bonds
            data.edge_attr = dense[off_diagonal]
        data.edge_index = pairs
        return data


def molecules(n_graphs, seed):
    """QM9-shaped molecules: a random tree of 3 to 29 atoms plus a few ring
    bonds, both directions, one of 4 bond types each."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(NUM_FEATURES, generator=g)
    out = []
    for _ in range(n_graphs):
        n = int(torch.randint(3, 30, (1,), generator=g))
        x = torch.zeros(n, NUM_FEATURES)
        x[torch.arange(n), torch.randint(0, 5, (n,), generator=g)] = 1.0       # the atom type, one-hot
        x[:, 5:] = torch.rand(n, NUM_FEATURES - 5, generator=g)
        pos = torch.randn(n, 3, generator=g) * (n ** (1.0 / 3))
        parent = torch.tensor([int(torch.randint(0, i, (1,), generator=g)) for i in range(1, n)], dtype=torch.long)
        a, b = torch.arange(1, n), parent
        extra = torch.randint(0, n, (2, max(n // 6, 1)), generator=g)
        extra = extra[:, extra[0] != extra[1]]
        a, b = torch.cat([a, extra[0]]), torch.cat([b, extra[1]])
        key = torch.unique(torch.minimum(a, b) * n + torch.maximum(a, b))       # each bond once
        a, b = key // n, key % n
        kind = F.one_hot(torch.randint(0, 4, (a.numel(),), generator=g), 4).float()
        y = (x @ w).mean() + 0.05 * n
        out.append(Data(x=x, pos=pos, edge_index=torch.stack([torch.cat([a, b]), torch.cat([b, a])]),
                        edge_attr=torch.cat([kind, kind]), y=y.view(1)))
    return out


ROUNDS = 3          # message-passing rounds, all with the one NNConv and the one GRU
EDGE_COLUMNS = 5    # 4 one-hot bond columns + the distance


def edge_network():
    """Edge columns -> the dim x dim matrix of a message; it ends in a Linear, so
    NNConv never builds the per-edge matrices."""
    return Sequential(Linear(EDGE_COLUMNS, 128), ReLU(), Linear(128, dim * dim))


class Net(torch.nn.Module):
    def __init__(self):
        super(Net, self).__init__()
        self.embed = Linear(NUM_FEATURES, dim)
        self.conv = NNConv(dim, dim, edge_network(), aggr="mean")
        self.gru = GRU(dim, dim)
        self.readout = Set2Set(dim, processing_steps=3)
        self.head = Sequential(Linear(2 * dim, dim), ReLU(), Linear(dim, 1))

    def message_pass(self, atoms, state, data):
        """One round: the mean of the edge-conditioned messages, then the GRU
        with the atoms' previous state (a sequence of length one)."""
        messages = F.relu(self.conv(atoms, data.edge_index, data.edge_attr))
        atoms, state = self.gru(messages.unsqueeze(0), state)
        return atoms.squeeze(0), state

    def forward(self, data):
        atoms = F.relu(self.embed(data.x))
        state = atoms.unsqueeze(0)
        for _ in range(ROUNDS):
            atoms, state = self.message_pass(atoms, state, data)
        molecule = self.readout(atoms, data.batch)                     # [graphs, 2 * dim]
        return self.head(molecule).view(-1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--graphs", type=int, default=6400)
    args = ap.parse_args(argv)
    transform = T.Compose([Complete(), T.Distance(norm=False)])
    dataset = [transform(d) for d in molecules(args.graphs, 0)]
    y = torch.cat([d.y for d in dataset])
    mean, std = y.mean(), y.std()
    for d in dataset:
        d.y = (d.y - mean) / std
    loader = DataLoader(dataset, batch_size=128, shuffle=True)
    device = torch.device("cuda:0")
    model = Net().to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=0.001)
    losses = []
    for epoch in range(args.epochs):
        model.train()
        for data in loader:
            data = data.to(device)
            optimizer.zero_grad()
            loss = F.mse_loss(model(data), data.y)
            loss.backward()
            optimizer.step()
            losses.append(float(loss.detach()))
            print("loss {:.6f}".format(losses[-1]))
        print("Epoch: {:02d}, loss {:.4f}".format(epoch + 1, losses[-1]))
    return losses


if __name__ == "__main__":
    main()
