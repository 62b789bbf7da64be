"""One ARMAConv layer (K = 3 stacks, C = 16, T = 2 shared-weight steps, dropout
0.25: the first layer of examples/arma.py), forward and forward + backward, in
three variants:

  fused     the layer's fused path: one launch per step over the stacked
            [N, K*C] layout (mi355_mp.ops.arma_propagate, csrc/mp_arma.hip)
  upstream  PyG 1.4.3's recipe in torch device ops: [K, E, C] messages, one
            index_add_ per step (ARMAConv.recipe)
  composed  the existing ops: fused_propagate over [N, K*C] rows, torch
            elementwise skip / bias / activation, bmm for the per-stack transform

at the example's Cora-shaped graph and the 100k-node / 1M-edge power-law graph
of tools/bench_dna.py, and at two power-law graphs between them.  Timed with device events after a
warm-up, in windows of at least --window seconds, the variants alternating
inside every repeat (median and max - min over the repeats); the peak device
memory of one forward + backward is recorded for each variant.

    python tools/bench_arma.py [--out profiles/arma_bench.json]
"""
import argparse
import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mi355_mp import _lib, ops  # noqa: E402
from mi355_mp.graph import graph_for  # noqa: E402
from mi355_mp.graphgen import cora_like, powerlaw_edge_index  # noqa: E402
from torch_geometric.nn import ARMAConv  # noqa: E402

K, C, T, DROPOUT = 3, 16, 2, 0.25
# (name, None = the example's graph, or (nodes, edges) of a power-law graph with 64 features)
WORKLOADS = [("arma_cora", None), ("arma_10k_100k", (10_000, 100_000)), ("arma_30k_300k", (30_000, 300_000)),
             ("arma_100k_1m", (100_000, 1_000_000))]


def composed(conv, x, ei):
    """The layer on the ops that existed before the fused step, the normalisation per call as in the others."""
    n = x.shape[0]
    graph = graph_for(ei, n, n, "target_to_source")
    lap = ops.arma_laplacian(graph)
    stack = lambda t: t.permute(1, 0, 2).reshape(n, K * C)  # noqa: E731
    y = stack(torch.matmul(x.unsqueeze(0), conv.ws[0]))
    for t in range(T):
        h = ops.fused_propagate(graph, y, ei, lap, "sum").view(n, K, C).permute(1, 0, 2)
        skip = F.dropout(x, p=conv.dropout, training=conv.training)
        h = F.relu(h + torch.matmul(skip.unsqueeze(0), conv.vs[0]) + conv.bias[0])
        if t + 1 < T:
            y = stack(torch.bmm(h, conv.ws[1]))
    return h.mean(dim=0)


def window_ms(step, min_s):
    """Mean ms per step over one window of at least min_s seconds (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, total = 0, 0.0
    batch = 1
    while total < min_s * 1e3:
        a.record()
        for _ in range(batch):
            step()
        b.record()
        b.synchronize()
        total += a.elapsed_time(b)
        n += batch
        batch = min(batch * 2, 64)
    return total / n


def peak_bytes(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    _lib.load()
    records = []
    for name, which in WORKLOADS:
        torch.manual_seed(0)
        if which is None:
            d = cora_like()
            ei, x = d["edge_index"].to(dev), d["x"].to(dev)
        else:
            ei = powerlaw_edge_index(which[0], which[1], seed=3, device=dev)
            x = torch.randn(which[0], 64, device=dev)
        n = x.shape[0]
        conv = ARMAConv(x.shape[1], C, num_stacks=K, num_layers=T, shared_weights=True, dropout=DROPOUT).to(dev)
        assert conv.fused(x)
        variants = {"fused": lambda: conv(x, ei, form="fused"),
                    "upstream": lambda: conv(x, ei, form="unfused"),
                    "composed": lambda: composed(conv, x, ei)}

        def make_steps(fn):
            def fwd():
                conv.eval()
                with torch.no_grad():
                    return fn()

            def train():
                conv.train()
                conv.zero_grad(set_to_none=True)
                fn().square().sum().backward()
            return fwd, train
        steps = {k: make_steps(v) for k, v in variants.items()}
        ref = steps["upstream"][0]()
        diff = {k: float((steps[k][0]() - ref).abs().max()) for k in steps if k != "upstream"}
        for fwd, train in steps.values():                              # warm-up (CSR builds, GEMM plans)
            for _ in range(3):
                fwd()
                train()
        torch.cuda.synchronize()
        times = {(k, p): [] for k in steps for p in ("fwd", "train")}
        for _ in range(args.repeats):
            for k, (fwd, train) in steps.items():
                times[(k, "fwd")].append(window_ms(fwd, args.window))
                times[(k, "train")].append(window_ms(train, args.window))
        rec = {"workload": name, "N": n, "E": int(ei.shape[1]), "F": int(x.shape[1]), "K": K, "C": C, "T": T,
               "dropout": DROPOUT, "max_abs_out": float(ref.abs().max()), "max_abs_diff_vs_upstream": diff,
               "source_hash": _lib.source_hash()}
        for (k, p), v in times.items():
            v = sorted(v)
            rec["%s_%s_ms" % (k, p)] = round(v[len(v) // 2], 4)
            rec["%s_%s_spread_ms" % (k, p)] = round(v[-1] - v[0], 4)
        for k, (_fwd, train) in steps.items():
            rec["%s_train_peak_bytes" % k] = peak_bytes(train)
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del conv, x
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0),
                       "window_s": args.window, "repeats": args.repeats, "records": records}, fh, indent=1)
            fh.write("\n")
    return records


if __name__ == "__main__":
    main()
