"""Writes tests/golden/spline/spline_kat.npz: known answers of the B-spline basis
(tests/_spline_ref.py) for fixed pseudo-coordinates, one entry set per
(D, degree) in {1,2,3}^2 with kernel sizes [5, 3, 4][:D] and open flags
[1, 0, 1][:D].  The file lives in its own directory: tests/test_oracle.py
recomputes every .npz directly under tests/golden/ with make_golden.compute,
which knows the scatter oracle's fixtures only.  Regenerate with

    python tests/golden/make_golden_spline.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _spline_ref as R  # noqa: E402

KS, OPEN = [5, 3, 4], [1, 0, 1]


def pseudo_for(D):
    g = torch.Generator().manual_seed(100 + D)
    u = torch.rand(24, D, generator=g)
    u[0] = 0.0
    u[1] = 1.0
    u[2] = 0.5
    u[3] = torch.tensor([1.0 / KS[d] for d in range(D)])
    return u


def main():
    out = {}
    for D in (1, 2, 3):
        u = pseudo_for(D)
        out["pseudo_d%d" % D] = u.numpy()
        for M in (1, 2, 3):
            ks = [max(k, M + o) for k, o in zip(KS[:D], OPEN[:D])]
            b, wi = R.basis(u, ks, OPEN[:D], M)
            out["basis_d%d_m%d" % (D, M)] = b.numpy()
            out["index_d%d_m%d" % (D, M)] = wi.numpy()
    np.savez_compressed(os.path.join(HERE, "spline", "spline_kat.npz"), **out)


if __name__ == "__main__":
    main()
