"""Writes tests/golden/glob/glob_kat.npz: a handful of tiny attention-readout
cases -- inputs (float32 draws of a seeded generator) and the float64 outputs of
the literal per-graph loop of tests/_glob_ref.py -- that tests/test_glob_host.py
checks the vectorised restatement against.  Run from the repository root:

    python tests/golden/make_golden_glob.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _glob_ref as R  # noqa: E402

# (name, graph sizes, C, mode)
CASES = [("q_small", [3, 1, 4], 3, "q"), ("q_empty", [0, 2, 0, 5, 0], 4, "q"), ("s_small", [2, 6], 5, "s"),
         ("s_empty", [0, 0, 3, 1, 0], 1, "s"), ("q_one", [7], 2, "q")]


def starts_of(sizes):
    return torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int64)


def inputs():
    g = torch.Generator().manual_seed(20260)
    t = {}
    for name, sizes, C, mode in CASES:
        n = sum(sizes)
        t[name + ".x"] = torch.randn(n, C, generator=g)
        t[name + (".q" if mode == "q" else ".score")] = (torch.randn(len(sizes), C, generator=g) if mode == "q"
                                                          else torch.randn(n, generator=g))
    return t


def answers(t, fn=R.readout_loop):
    out = {}
    for name, sizes, C, mode in CASES:
        kw = {"q": t[name + ".q"]} if mode == "q" else {"score": t[name + ".score"]}
        r, e, m, den, a = fn(t[name + ".x"], starts_of(sizes), **kw)
        for k, v in (("r", r), ("e", e), ("m", m), ("den", den), ("a", a)):
            out["%s.out.%s" % (name, k)] = v.detach()
    return out


if __name__ == "__main__":
    t = inputs()
    arrays = {k: v.numpy() for k, v in t.items()}
    arrays.update({k: v.numpy() for k, v in answers(t).items()})
    path = os.path.join(ROOT, "tests", "golden", "glob", "glob_kat.npz")
    np.savez(path, **arrays)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(arrays), os.path.getsize(path)))
