"""Writes tests/golden/link/link_kat.npz: known answers of the link-prediction
restatement (tests/_link_ref.py) -- a directed graph on 13 nodes with repeated edges
and self loops, a path, and a complete graph minus one pair: the sampler's key
tables and its draws in the full, upper and row modes under two seeds, with and
without the loop rewrite of GAE.recon_loss, to_undirected, and for a small z the
scores, both sides' loss terms and coefficients, the gradient of z, and ROC-AUC /
average precision of tied scores.  The file lives in its own directory (see
make_golden_spline.py).  Regenerate with

    python tests/golden/make_golden_link.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _link_ref as R  # noqa: E402

N = 13
SEEDS = (7, 0x9E3779B97F4A7C15)
NAMES = ("edges", "path", "almost", "z", "labels", "scores")


def inputs():
    rng = np.random.default_rng(47)
    edges = rng.integers(0, N, (2, 40)).astype(np.int64)
    edges[:, 5] = edges[:, 4]                       # a repeated edge
    edges[1, 9] = edges[0, 9]                       # a self loop
    path = np.asarray([[0, 1, 2, 3], [1, 2, 3, 4]], dtype=np.int64)
    full = np.asarray([(i, j) for i in range(6) for j in range(6) if (i, j) != (4, 2)], dtype=np.int64).T
    z = (rng.integers(-8, 9, (N, 5)) / 4.0).astype(np.float32)
    labels = np.asarray([1, 0, 1, 1, 0, 0, 1, 0], dtype=np.int64)
    scores = np.asarray([0.9, 0.9, 0.5, 0.4, 0.4, 0.1, 0.4, 0.9], dtype=np.float64)
    return edges, path, full, z, labels, scores


def answers(edges, path, almost, z, labels, scores):
    out = {}
    for name, ei, n in (("edges", edges, N), ("path", path, 5), ("almost", almost, 6)):
        for upper in (False, True):
            tag = "%s_%s" % (name, "upper" if upper else "full")
            out[tag + "_keys"] = np.asarray(R.key_table(ei[0], ei[1], n, upper)[0], dtype=np.int64)
            for q, seed in enumerate(SEEDS):
                out["%s_s%d" % (tag, q)] = R.negative_sample(ei[0], ei[1], n, seed, upper=upper)
        out[name + "_loops_s0"] = R.negative_sample(ei[0], ei[1], n, SEEDS[0], loops=True)
        out[name + "_rows_s0"] = R.structured_negative_sample(ei[0], ei[1], n, SEEDS[0])
        out[name + "_undirected"] = R.to_undirected(ei, n)
    out["edges_full_17"] = R.negative_sample(edges[0], edges[1], N, SEEDS[1], num_neg_samples=17)
    v = R.score(z, edges[0], edges[1])
    out["v"] = v
    for positive in (True, False):
        t, coef = R.loss_terms(v, positive)
        side = "pos" if positive else "neg"
        out["t_" + side], out["coef_" + side] = t, coef
        out["dz_" + side] = R.grad_z(z, edges[0], edges[1], coef)
    out["auc_ap"] = np.asarray([R.roc_auc(labels, scores), R.average_precision(labels, scores)])
    return out


def main():
    ins = inputs()
    out = dict(zip(NAMES, ins))
    out.update(answers(*ins))
    os.makedirs(os.path.join(HERE, "link"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "link", "link_kat.npz"), **out)


if __name__ == "__main__":
    main()
