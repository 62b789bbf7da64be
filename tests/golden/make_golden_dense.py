"""Writes tests/golden/dense/dense_kat.npz: a handful of tiny dense_diff_pool and
dense mean-aggregation cases -- inputs (float32 draws of a seeded generator) and
the float64 outputs of the literal per-entry loops of tests/_dense_ref.py -- that
tests/test_dense_host.py checks the vectorised restatement against, and one case
worked by hand.  Run from the repository root:

    python tests/golden/make_golden_dense.py

The hand case: one graph of two nodes, s rows (0, ln 3) so P = (1/4, 3/4) for
both, x = (4, 8), adj = [[0, 1], [1, 0]]:
    out = P^T x = (3, 9);  T = adj P = P;  out_adj = P^T T = [[1/8, 3/8], [3/8, 9/8]]
    p_i . p_j = 1/16 + 9/16 = 5/8 for every pair, so
    q = 2 (0 - 5/8)^2 + 2 (1 - 5/8)^2 = 17/16,  link = sqrt(17/16) / 4 = sqrt(17) / 16
    h = 2 (ln 4 / 4 + 3 ln(4/3) / 4),  ent = h / 2 = ln 4 - 3 ln 3 / 4
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _dense_ref as R  # noqa: E402

# (name, B, N, C, F, mask: None | "part" | "empty_graph", adj: "01" | "real")
CASES = [("small", 2, 4, 3, 2, None, "01"), ("masked", 3, 5, 2, 3, "part", "01"),
         ("empty_graph", 2, 3, 2, 1, "empty_graph", "real"), ("one_node", 1, 1, 1, 1, None, "real"),
         ("pooled", 1, 3, 4, 2, None, "real")]
KEYS = ("out", "out_adj", "link", "ent", "P", "T", "V", "q", "h")


def hand():
    """inputs and the answers worked in the module docstring"""
    t = {"hand.x": torch.tensor([[[4.0], [8.0]]], dtype=torch.float64),
         "hand.adj": torch.tensor([[[0.0, 1.0], [1.0, 0.0]]], dtype=torch.float64),
         "hand.s": torch.tensor([[[0.0, math.log(3.0)], [0.0, math.log(3.0)]]], dtype=torch.float64)}
    want = {"hand.out.out": torch.tensor([[[3.0], [9.0]]], dtype=torch.float64),
            "hand.out.out_adj": torch.tensor([[[0.125, 0.375], [0.375, 1.125]]], dtype=torch.float64),
            "hand.out.P": torch.tensor([[[0.25, 0.75], [0.25, 0.75]]], dtype=torch.float64),
            "hand.out.q": torch.tensor([17.0 / 16.0], dtype=torch.float64),
            "hand.out.link": torch.tensor(math.sqrt(17.0) / 16.0, dtype=torch.float64),
            "hand.out.ent": torch.tensor(math.log(4.0) - 0.75 * math.log(3.0), dtype=torch.float64)}
    return t, want


def mask_of(kind, B, N):
    if kind is None:
        return None
    m = torch.ones((B, N), dtype=torch.bool)
    if kind == "part":
        for b in range(B):
            m[b, N - b:] = False            # graph 0 is full, graph b has b padding rows
    else:
        m[0] = False                        # every node of graph 0 is masked
        m[1, -1] = False
    return m


def inputs():
    g = torch.Generator().manual_seed(20261)
    t = {}
    for name, B, N, C, F, mk, kind in CASES:
        t[name + ".x"] = torch.randn(B, N, F, generator=g)
        a = torch.randn(B, N, N, generator=g)
        t[name + ".adj"] = a if kind == "real" else (a > 0.3).float()
        t[name + ".s"] = torch.randn(B, N, C, generator=g)
    return t


def answers(t, fn=R.diff_pool_loop, agg=R.mean_agg_loop):
    out = {}
    for name, B, N, C, F, mk, kind in CASES:
        r = fn(t[name + ".x"], t[name + ".adj"], t[name + ".s"], mask_of(mk, B, N))
        for k in KEYS:
            out["%s.out.%s" % (name, k)] = r[k].detach()
        for loop in (0, 1):
            a, d = agg(t[name + ".x"], t[name + ".adj"], bool(loop))
            out["%s.agg%d" % (name, loop)] = a.detach()
            out["%s.deg%d" % (name, loop)] = d.detach()
    return out


if __name__ == "__main__":
    t = inputs()
    ht, hw = hand()
    arrays = {k: v.numpy() for k, v in t.items()}
    arrays.update({k: v.numpy() for k, v in answers(t).items()})
    arrays.update({k: v.numpy() for k, v in ht.items()})
    arrays.update({k: v.numpy() for k, v in hw.items()})
    path = os.path.join(ROOT, "tests", "golden", "dense", "dense_kat.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, **arrays)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(arrays), os.path.getsize(path)))
