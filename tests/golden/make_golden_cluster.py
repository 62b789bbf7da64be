"""Writes tests/golden/cluster/cluster_kat.npz: known answers of the cluster
pooling restatement (tests/_cluster_ref.py) for one small batch -- three graphs
of 40 random points in [0, 28)^2 with quantised features, 8 edges per node --
under the reference example's three voxel settings, and max_pool of the first.
The file lives in its own directory (see make_golden_spline.py).  Regenerate with

    python tests/golden/make_golden_cluster.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _cluster_ref as R  # noqa: E402

SETTINGS = [(5, 0, 28), (7, 0, 28), (14, 0, 27.99)]


def inputs():
    g = torch.Generator().manual_seed(11)
    n_g, G = 40, 3
    n = n_g * G
    pos = torch.rand(n, 2, generator=g) * 28
    batch = torch.arange(G).repeat_interleave(n_g)
    x = torch.randint(-2, 3, (n, 3), generator=g).float() * 0.5
    x[::17, 1] = -20000.0
    ei = torch.cat([torch.randint(0, n_g, (2, 8 * n_g), generator=g) + k * n_g for k in range(G)], dim=1)
    attr = torch.rand(ei.size(1), 2, generator=g)
    return pos, batch, x, ei, attr


def main():
    pos, batch, x, ei, attr = inputs()
    out = {"pos": pos.numpy(), "batch": batch.numpy(), "x": x.numpy(), "edge_index": ei.numpy(),
           "edge_attr": attr.numpy()}
    for i, (size, start, end) in enumerate(SETTINGS):
        out["key_%d" % i] = R.voxel_grid(pos, batch, size, start, end).numpy()
    out["key_auto"] = R.voxel_grid(pos, batch, [5, 0.1]).numpy()
    p = R.pool(torch.from_numpy(out["key_0"]), x, pos, batch, ei, attr)
    for k in ("inv", "perm", "x", "arg", "pos", "batch", "edge_index", "edge_attr", "edge_slot"):
        out["pool_" + k] = p[k].numpy()
    os.makedirs(os.path.join(HERE, "cluster"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "cluster", "cluster_kat.npz"), **out)


if __name__ == "__main__":
    main()
