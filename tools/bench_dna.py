"""DNAConv layer bench: the fused path against upstream's recipe in torch device
ops -- x_i[:, -1:] and x_j [E, T, C] gathered per edge, the grouped Linears per
edge, the restricted softmax, dropout, norm, index_add_ -- and against this
repository's generic MessagePassing path (the same message, native gathers and
segmented reduce).  All three start from the cached normalised edge list.

Shapes: the layer of examples/dna.py (128 channels, 8 heads, 16 groups, dropout
0.8) on its Cora-shaped graph (2708 nodes, about 13 k edges with the self loops)
at T = 1 and T = 5 (the first and the last layer of the stack), and the same
layer on a power-law graph of 100 k nodes and 1 M edges (mi355_mp.graphgen).

Per variant: forward alone (eval, no autograd) and forward + backward of one
layer in training mode (loss = sum of squares, gradients for x and every
parameter), timed with device events after a warm-up, in windows of at least
--window seconds, the variants alternating inside every repeat (median and max -
min over the repeats), and the peak device memory of one forward + backward
above what was allocated before it.  One JSON line per shape; --out also writes
them to a file with the native source hash.  The bar: the fused path is not
slower forward + backward than the upstream recipe by more than the two spreads
together.

    python tools/bench_dna.py [--out profiles/dna_bench.json]
"""
import argparse
import importlib.util
import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402

from mi355_mp import _lib  # noqa: E402
from mi355_mp.graphgen import powerlaw_edge_index  # noqa: E402
from torch_geometric.nn import DNAConv  # noqa: E402

CHANNELS, HEADS, GROUPS, DROPOUT = 128, 8, 16, 0.8
# (name, graph, T)
WORKLOADS = [("dna_cora_t1", "cora", 1), ("dna_cora_t5", "cora", 5), ("dna_100k_1m_t1", "large", 1),
             ("dna_100k_1m_t5", "large", 5)]


def example_graph(dev):
    spec = importlib.util.spec_from_file_location("example_dna", os.path.join(_ROOT, "examples", "dna.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.graph(mod.CORA_NODES, 0)[1].to(dev), mod.CORA_NODES


def upstream(conv, x, edge_index, norm):
    """PyG 1.4.3's DNAConv message and aggregation in plain torch device ops."""
    src, dst = edge_index[0], edge_index[1]
    x_i, x_j = x[dst][:, -1:], x[src]
    out = conv.multi_head(x_i, x_j, x_j)
    msg = norm.view(-1, 1) * out.squeeze(1)
    return torch.zeros(x.shape[0], msg.shape[1], device=msg.device).index_add_(0, dst, msg)


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
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    _lib.load()
    only = set(args.only.split(",")) if args.only else None
    graphs = {}
    records = []
    for name, which, T in WORKLOADS:
        if only and name not in only:
            continue
        if which not in graphs:
            graphs[which] = example_graph(dev) if which == "cora" else \
                (powerlaw_edge_index(100_000, 1_000_000, seed=3, device=dev), 100_000)
        ei, n = graphs[which]
        torch.manual_seed(0)
        conv = DNAConv(CHANNELS, HEADS, GROUPS, dropout=DROPOUT, cached=True).to(dev)
        x = torch.randn(n, T, CHANNELS, device=dev, requires_grad=True)
        with torch.no_grad():
            conv.eval()
            conv(x, ei)                                                 # fills the cache: the normalised edge list
        ei2, norm = conv.cached_result
        assert conv._fused_ok(x, ei2, norm)
        variants = {"upstream": lambda: upstream(conv, x, ei2, norm),
                    "generic": lambda: conv.propagate(ei2, x=x, norm=norm),
                    "fused": lambda: conv(x, ei)}

        def make_steps(fn):
            def fwd():
                conv.eval()
                with torch.no_grad():
                    fn()

            def train():
                conv.train()
                conv.zero_grad(set_to_none=True)
                x.grad = None
                fn().square().sum().backward()
            return fwd, train
        steps = {k: make_steps(v) for k, v in variants.items()}
        with torch.no_grad():
            conv.eval()
            ref = variants["upstream"]()
            diff = {k: float((variants[k]() - ref).abs().max()) for k in variants if k != "upstream"}
            scale = float(ref.abs().max())
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
        rec = {"workload": name, "N": n, "E": int(ei2.shape[1]), "T": T, "C": CHANNELS, "H": HEADS, "G": GROUPS,
               "dropout": DROPOUT, "max_abs_out": scale, "max_abs_diff_vs_upstream": diff,
               "one_E_T_C_array_bytes": int(ei2.shape[1]) * T * CHANNELS * 4, "source_hash": _lib.source_hash()}
        for (k, p), v in times.items():
            v = sorted(v)
            rec["%s_%s_ms" % (k, p)] = round(v[len(v) // 2], 4)
            rec["%s_%s_spread_ms" % (k, p)] = round(v[-1] - v[0], 4)
        for k, (_fwd, train) in steps.items():
            rec["%s_train_peak_bytes" % k] = peak_bytes(train)
        slack = rec["fused_train_spread_ms"] + rec["upstream_train_spread_ms"]
        rec["bar_met"] = rec["fused_train_ms"] <= rec["upstream_train_ms"] + slack
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
