"""Writes tests/golden/gmm/gmm_kat.npz: known answers of the GMMConv
restatement (tests/_gmm_ref.py) on one small fixed graph -- the shared-Gaussian
layer for add / mean / max in both flows, the separate-Gaussian layer, and the
three kernel contracts (bins, gather, param_grad).  The file lives in its own
directory: tests/test_oracle.py recomputes every .npz directly under
tests/golden/ with make_golden.compute, which knows the scatter oracle's
fixtures only.  Regenerate with

    python tests/golden/make_golden_gmm.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _gmm_ref as R  # noqa: E402

N, E, K, D, CIN, COUT = 9, 30, 3, 2, 2, 5


def inputs():
    g = torch.Generator().manual_seed(2025)
    ei = torch.randint(0, N - 2, (2, E), generator=g)                  # nodes 7, 8 isolated
    sign = lambda *s: torch.randint(0, 2, s, generator=g).float() * 2 - 1   # noqa: E731
    t = {"edge_index": ei, "pseudo": torch.rand(E, D, generator=g), "x": torch.randn(N, CIN, generator=g),
         "g": torch.randn(CIN, K * COUT, generator=g), "mu": torch.rand(K, D, generator=g),
         "sigma": (torch.rand(K, D, generator=g) + 0.5) * sign(K, D),
         "mu_sep": torch.rand(CIN, COUT, K, D, generator=g),
         "sigma_sep": (torch.rand(CIN, COUT, K, D, generator=g) + 0.5) * sign(CIN, COUT, K, D),
         "root": torch.randn(CIN, COUT, generator=g), "bias": torch.randn(COUT, generator=g),
         "y": torch.randn(N, K * COUT, generator=g), "dz": torch.randn(N, K * CIN, generator=g),
         "scale": torch.rand(N, generator=g) + 0.5}
    return t


def answers(t):
    ei = t["edge_index"]
    out = {"weights": R.weights(t["pseudo"], t["mu"], t["sigma"])}
    for aggr in ("add", "mean", "max"):
        for flow, tag in (("source_to_target", "s2t"), ("target_to_source", "t2s")):
            out["layer_%s_%s" % (aggr, tag)] = R.gmm_conv(t["x"], ei, t["pseudo"], t["g"], t["mu"], t["sigma"], K,
                                                          t["root"], t["bias"], aggr, flow)
    out["layer_add_plain"] = R.gmm_conv(t["x"], ei, t["pseudo"], t["g"], t["mu"], t["sigma"], K, None, None, "add")
    out["layer_sep_mean"] = R.gmm_conv(t["x"], ei, t["pseudo"], t["g"], t["mu_sep"], t["sigma_sep"], K, t["root"],
                                       t["bias"], "mean")
    out["bins"] = R.bins(ei[1], ei[0], N, t["pseudo"], t["mu"], t["sigma"], t["x"], t["scale"])
    out["gather"] = R.gather(ei[1], ei[0], N, t["pseudo"], t["mu"], t["sigma"], t["y"], COUT, t["scale"], t["bias"])
    dmu, dsigma, dpseudo = R.param_grad(ei[1], ei[0], t["pseudo"], t["mu"], t["sigma"], t["dz"], t["x"])
    out.update({"dmu": dmu, "dsigma": dsigma, "dpseudo": dpseudo})
    return out


def main():
    t = inputs()
    out = {k: v.numpy() for k, v in t.items()}
    out.update({k: v.numpy() for k, v in answers(t).items()})
    os.makedirs(os.path.join(HERE, "gmm"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "gmm", "gmm_kat.npz"), **out)


if __name__ == "__main__":
    main()
