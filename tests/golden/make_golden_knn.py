"""Writes tests/golden/knn/knn_kat.npz: known answers of the nearest-neighbour
restatement (tests/_knn_ref.py) -- a 4 x 4 integer lattice queried from its own
points and from cell centres (ties everywhere: they go to the lower index), a
cloud of 24 rows that holds only 5 distinct points, and a batch in which graph 1
is missing from x and graph 3 from y, on a half-unit lattice -- knn at k = 1, 3 and
16, knn_graph with and without loops in both flows, and nearest.  The file lives
in its own directory (see make_golden_spline.py).  Regenerate with

    python tests/golden/make_golden_knn.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _knn_ref as R  # noqa: E402

X_SIZES = (9, 0, 14, 6)
Y_SIZES = (4, 3, 5, 0)
NAMES = ("lattice", "centres", "dups", "pos", "y", "batch", "batch_y")


def inputs():
    rng = np.random.default_rng(43)
    gx, gy = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
    lattice = np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.float32)
    centres = (lattice[[0, 1, 5, 10]] + 0.5).astype(np.float32)           # four equidistant corners each
    dups = rng.integers(0, 2, (5, 3)).astype(np.float32)[rng.integers(0, 5, 24)]
    pos = (rng.integers(0, 4, (sum(X_SIZES), 3)) * 0.5).astype(np.float32)
    y = (rng.integers(0, 4, (sum(Y_SIZES), 3)) * 0.5).astype(np.float32)
    batch = np.repeat(np.arange(len(X_SIZES)), X_SIZES).astype(np.int64)
    batch_y = np.repeat(np.arange(len(Y_SIZES)), Y_SIZES).astype(np.int64)
    return lattice, centres, dups, pos, y, batch, batch_y


def answers(lattice, centres, dups, pos, y, batch, batch_y):
    out = {}
    for k in (1, 3, 16):
        out["lattice_self_k%d" % k] = R.knn(lattice, lattice, k)
        out["lattice_centres_k%d" % k] = R.knn(lattice, centres, k)
        out["dups_k%d" % k] = R.knn(dups, dups, k)
        out["batch_k%d" % k] = R.knn(pos, y, k, batch, batch_y)
    out["graph_k3"] = R.knn_graph(pos, 3, batch)
    out["graph_k3_loop_t2s"] = R.knn_graph(pos, 3, batch, True, "target_to_source")
    out["graph_dups_k2"] = R.knn_graph(dups, 2)
    out["nearest_lattice"] = R.nearest(centres, lattice)
    has_x = np.isin(batch_y, np.unique(batch))
    out["nearest_batch"] = R.nearest(y[has_x], pos, batch_y[has_x], batch)
    return out


def main():
    ins = inputs()
    out = dict(zip(NAMES, ins))
    out.update(answers(*ins))
    os.makedirs(os.path.join(HERE, "knn"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "knn", "knn_kat.npz"), **out)


if __name__ == "__main__":
    main()
