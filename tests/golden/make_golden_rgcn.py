"""Writes tests/golden/rgcn/rgcn_kat.npz: known answers of the RGCNConv
restatement (tests/_rgcn_ref.py) on one small fixed graph -- the featured and
the featureless layer in both flows, with and without edge_norm, root and
bias, and the three kernel contracts (bins, gather, att_grad).  The file lives
in its own directory: tests/test_oracle.py recomputes every .npz directly under
tests/golden/ with make_golden.compute, which knows the scatter oracle's
fixtures only.  Regenerate with

    python tests/golden/make_golden_rgcn.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _rgcn_ref as R  # noqa: E402

N, E, NREL, B, CIN, COUT = 9, 30, 4, 3, 2, 5


def inputs():
    g = torch.Generator().manual_seed(2025)
    ei = torch.randint(0, N - 2, (2, E), generator=g)                  # nodes 7, 8 isolated
    t = {"edge_index": ei, "edge_type": torch.randint(0, NREL - 1, (E,), generator=g),   # relation 3 without edges
         "edge_norm": torch.rand(E, generator=g) + 0.5, "x": torch.randn(N, CIN, generator=g),
         "basis": torch.randn(B, CIN, COUT, generator=g), "att": torch.randn(NREL, B, generator=g),
         "root": torch.randn(CIN, COUT, generator=g), "bias": torch.randn(COUT, generator=g),
         "basis_n": torch.randn(B, N, COUT, generator=g), "root_n": torch.randn(N, COUT, generator=g),
         "y": torch.randn(N, B, COUT, generator=g), "dz": torch.randn(N, B, CIN, generator=g)}
    return t


def answers(t):
    ei, et, en = t["edge_index"], t["edge_type"], t["edge_norm"]
    out = {}
    for flow, tag in (("source_to_target", "s2t"), ("target_to_source", "t2s")):
        out["layer_%s" % tag] = R.rgcn_conv(t["x"], ei, et, en, t["basis"], t["att"], t["root"], t["bias"], flow)
        out["featureless_%s" % tag] = R.rgcn_conv(None, ei, et, en, t["basis_n"], t["att"], t["root_n"], t["bias"],
                                                  flow)
    out["layer_plain"] = R.rgcn_conv(t["x"], ei, et, None, t["basis"], t["att"])
    out["featureless_plain"] = R.rgcn_conv(None, ei, et, None, t["basis_n"], t["att"])
    out["bins"] = R.bins(ei[1], ei[0], N, et, en, t["att"], t["x"])
    out["gather"] = R.gather(ei[1], ei[0], N, et, en, t["att"], t["y"], t["bias"])
    out["att_grad"] = R.att_grad(et, en, ei[1], ei[0], t["dz"], t["x"], NREL)
    return out


def main():
    t = inputs()
    out = {k: v.numpy() for k, v in t.items()}
    out.update({k: v.numpy() for k, v in answers(t).items()})
    os.makedirs(os.path.join(HERE, "rgcn"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "rgcn", "rgcn_kat.npz"), **out)


if __name__ == "__main__":
    main()
