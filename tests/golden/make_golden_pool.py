"""Writes tests/golden/pool/pool_kat.npz: known answers of the per-graph top-k
selection (tests/_pool_ref.py, the stable restatement) for a fixed batch of
graph sizes, two score vectors (distinct values; five repeated values with
+-0.0, +-inf and NaN) and the six ratios of the GPU tests, plus filter_adj of
one of the selections on a fixed edge list.  The file lives in its own
directory (see make_golden_spline.py).  Regenerate with

    python tests/golden/make_golden_pool.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _pool_ref as R  # noqa: E402

SIZES = [5, 0, 1, 2, 25, 50, 63, 64, 65, 0, 126, 130]
RATIOS = [0.8, 0.5, 0.3, 0.6, 0.001, 1.0]
FIVE = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan")])


def inputs():
    g = torch.Generator().manual_seed(7)
    n = sum(SIZES)
    distinct = R.distinct_scores(n, g)
    tied = FIVE[torch.randint(0, 5, (n,), generator=g)]
    ei = torch.randint(0, n, (2, 900), generator=g)
    return distinct, tied, ei


def main():
    distinct, tied, ei = inputs()
    out = {"sizes": np.array(SIZES), "ratios": np.array(RATIOS), "distinct": distinct.numpy(), "tied": tied.numpy(),
           "edge_index": ei.numpy()}
    for i, r in enumerate(RATIOS):
        for name, s in (("distinct", distinct), ("tied", tied)):
            perm, starts = R.topk_stable(s, r, SIZES)
            out["perm_%s_%d" % (name, i)] = perm.numpy()
            out["starts_%s_%d" % (name, i)] = starts.numpy()
    perm, _ = R.topk_stable(tied, 0.5, SIZES)
    fe, _, pos = R.filter_adj(ei, None, perm, sum(SIZES))
    out["filter_index"] = fe.numpy()
    out["filter_pos"] = pos.numpy()
    os.makedirs(os.path.join(HERE, "pool"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "pool", "pool_kat.npz"), **out)


if __name__ == "__main__":
    main()
