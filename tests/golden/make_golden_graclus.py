"""Writes tests/golden/graclus/graclus_kat.npz: known answers of the graclus
restatement (tests/_graclus_ref.py) for one small batch -- three graphs of 20
nodes, 5 random edges per node (loops and repeated pairs among them), weights
quantised to five values -- the priorities of its first 8 entries, and the
clusters and round counts for two seeds, weighted and unweighted.  The file
lives in its own directory (see make_golden_spline.py).  Regenerate with

    python tests/golden/make_golden_graclus.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _graclus_ref as R  # noqa: E402

SEEDS = (0, 1)
N_PRIORITIES = 8


def inputs():
    rng = np.random.default_rng(23)
    n_g, G = 20, 3
    ei = np.concatenate([rng.integers(0, n_g, (2, 5 * n_g)) + k * n_g for k in range(G)], axis=1).astype(np.int64)
    w = (rng.integers(0, 5, ei.shape[1]) * 0.25 - 0.5).astype(np.float32)
    return ei, w, n_g * G


def answers(ei, w, n):
    out = {}
    for seed in SEEDS:
        keys = [k for k in R.priorities(ei, w, seed)[:N_PRIORITIES]]
        out["priorities_%d" % seed] = np.asarray([(0, 0, 0, 0) if k is None else k for k in keys], dtype=np.uint64)
        for name, ww in (("weighted", w), ("unweighted", None)):
            cluster, rounds = R.handshake(ei, ww, n, seed)
            out["cluster_%s_%d" % (name, seed)] = cluster
            out["rounds_%s_%d" % (name, seed)] = np.asarray(rounds, dtype=np.int64)
    return out


def main():
    ei, w, n = inputs()
    out = {"edge_index": ei, "weight": w, "num_nodes": np.asarray(n, dtype=np.int64)}
    out.update(answers(ei, w, n))
    os.makedirs(os.path.join(HERE, "graclus"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "graclus", "graclus_kat.npz"), **out)


if __name__ == "__main__":
    main()
