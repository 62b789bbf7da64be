"""Writes tests/golden/nnconv/nnconv_kat.npz: known answers of the NNConv
restatement (tests/_nnconv_ref.py) on one small fixed graph -- the layer for
add / mean / max in both flows, and the three kernel contracts (bins, gather,
edge_grad).  The file lives in its own directory: tests/test_oracle.py
recomputes every .npz directly under tests/golden/ with make_golden.compute,
which knows the scatter oracle's fixtures only.  Regenerate with

    python tests/golden/make_golden_nnconv.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _nnconv_ref as R  # noqa: E402

N, E, H, CIN, COUT = 9, 30, 3, 2, 5


def inputs():
    g = torch.Generator().manual_seed(2024)
    ei = torch.randint(0, N - 2, (2, E), generator=g)                  # nodes 7, 8 isolated
    t = {"edge_index": ei, "h": torch.randn(E, H, generator=g), "x": torch.randn(N, CIN, generator=g),
         "head_w": torch.randn(CIN * COUT, H, generator=g), "head_b": torch.randn(CIN * COUT, generator=g),
         "root": torch.randn(CIN, COUT, generator=g), "bias": torch.randn(COUT, generator=g),
         "y": torch.randn(N, (H + 1) * COUT, generator=g), "dz": torch.randn(N, (H + 1) * CIN, generator=g),
         "scale": torch.rand(N, generator=g) + 0.5}
    return t


def answers(t):
    ei = t["edge_index"]
    out = {}
    for aggr in ("add", "mean", "max"):
        for flow, tag in (("source_to_target", "s2t"), ("target_to_source", "t2s")):
            out["layer_%s_%s" % (aggr, tag)] = R.nn_conv(t["x"], ei, t["h"], t["head_w"], t["head_b"], CIN, COUT,
                                                         t["root"], t["bias"], aggr, flow)
    out["layer_add_plain"] = R.nn_conv(t["x"], ei, t["h"], t["head_w"], None, CIN, COUT, None, None, "add")
    out["bins"] = R.bins(ei[1], ei[0], N, t["h"], t["x"], t["scale"])
    out["gather"] = R.gather(ei[1], ei[0], N, t["h"], t["y"], COUT, t["scale"], t["bias"])
    out["edge_grad"] = R.edge_grad(ei[1], ei[0], t["dz"], t["x"], H)
    return out


def main():
    t = inputs()
    out = {k: v.numpy() for k, v in t.items()}
    out.update({k: v.numpy() for k, v in answers(t).items()})
    os.makedirs(os.path.join(HERE, "nnconv"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "nnconv", "nnconv_kat.npz"), **out)


if __name__ == "__main__":
    main()
