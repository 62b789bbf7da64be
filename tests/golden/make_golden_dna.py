"""Writes tests/golden/dna/dna_kat.npz: known answers of the DNAConv
restatement (tests/_dna_ref.py) on one small fixed graph -- the layer in both
flows with and without edge weights and a dropout mask, the GCN normalisation,
and the kernel contracts (attention, its backward, the sum |terms| scale).  The
file lives in its own directory: tests/test_oracle.py recomputes every .npz
directly under tests/golden/ with make_golden.compute, which knows the scatter
oracle's fixtures only.  Regenerate with

    python tests/golden/make_golden_dna.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _dna_ref as R  # noqa: E402

N, E, T, C, H, G = 9, 30, 3, 12, 3, 2
P = 0.5


def inputs():
    g = torch.Generator().manual_seed(2026)
    ei = torch.randint(0, N - 2, (2, E), generator=g)                  # nodes 7, 8 isolated (their loops remain)
    ei[:, 3] = 2                                                       # two existing self loops on node 2:
    ei[:, 11] = 2                                                      # the later one's weight stays
    t = {"edge_index": ei, "edge_weight": torch.rand(E, generator=g) + 0.5, "x": torch.randn(N, T, C, generator=g)}
    for name in ("wq", "wk", "wv"):
        t[name] = torch.randn(G, C // G, C // G, generator=g) / (C // G) ** 0.5
    for name in ("bq", "bk", "bv"):
        t[name] = torch.randn(C, generator=g)
    t["gout"] = torch.randn(N, C, generator=g)
    n_loops = int((ei[0] == ei[1]).sum())
    t["keep"] = torch.rand(E - n_loops + N, H, T, generator=g) >= P
    return t


def answers(t):
    ei = t["edge_index"]
    prm = {k: t[k] for k in R.PARAMS}
    out = {}
    ei_w, norm_w = R.gcn_norm(ei, N, t["edge_weight"])
    ei_1, norm_1 = R.gcn_norm(ei, N)
    assert torch.equal(ei_w, ei_1)
    out["norm_weighted"], out["norm_plain"] = norm_w, norm_1
    for flow, tag in (("source_to_target", "s2t"), ("target_to_source", "t2s")):
        out["layer_%s" % tag] = R.dna_conv(t["x"], ei_w, norm_w, prm, H, flow)
        out["layer_drop_%s" % tag] = R.dna_conv(t["x"], ei_w, norm_w, prm, H, flow, keep=t["keep"], p=P)
    out["layer_plain"] = R.dna_conv(t["x"], ei_1, norm_1, prm, H)
    out["layer_no_bias"] = R.dna_conv(t["x"], ei_1, norm_1, {k: (v if k[0] == "w" else None) for k, v in prm.items()}, H)
    q, k, v = R.project(t["x"].double(), {n: p.double() for n, p in prm.items()})
    dst, src = ei_w[1], ei_w[0]
    out["attention"] = R.attention(q, k, v, norm_w, dst, src, N, H)
    out["attention_abs"] = R.attention_abs(q, k, v, norm_w, dst, src, N, H, keep=t["keep"], p=P)
    for tag, kw in (("", {}), ("_drop", {"keep": t["keep"], "p": P})):
        dq, dk, dv = R.attention_backward(q, k, v, norm_w, dst, src, N, H, t["gout"], **kw)
        out["dq" + tag], out["dk" + tag], out["dv" + tag] = dq, dk, dv
    return out


def main():
    t = inputs()
    out = {k: v.numpy() for k, v in t.items()}
    out.update({k: v.numpy() for k, v in answers(t).items()})
    os.makedirs(os.path.join(HERE, "dna"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "dna", "dna_kat.npz"), **out)


if __name__ == "__main__":
    main()
