"""RGCNConv layer bench: the fused path (each forced form and the form the layer
picks) against upstream's recipe in torch device ops -- att @ basis, then
index_select(w, 0, edge_type) [E, Cin, Cout] -> bmm with x[j] -> index_add_
(x = None: the [R * N, Cout] table, gathered by type * N + j) -- and against
this repository's generic MessagePassing path (the same message, native gathers
and segmented reduce).

Shapes: the two layers of examples/rgcn.py on its MUTAG-shaped entity graph
(23 644 nodes, 148 454 edges, 46 relations, 30 bases: the featureless N -> 16
layer and the 16 -> 2 layer) and a 64 -> 64 layer on the same graph.

Per variant: forward alone (no autograd) and forward + backward of one layer
(loss = sum of squares, gradients for x and every parameter), timed with device
events after a warm-up, in windows of at least --window seconds, the variants
alternating inside every repeat (median and max - min over the repeats), and
the peak device memory of one forward + backward above what was allocated
before it.  One JSON line per shape; --out also writes them to a file with the
native source hash.  The bar: the layer's pick is not slower forward + backward
than the upstream recipe by more than the two spreads together.

    python tools/bench_rgcn.py [--out profiles/rgcn_bench.json]
"""
import argparse
import importlib.util
import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402

from mi355_mp import _lib, ops  # noqa: E402
from torch_geometric.nn import RGCNConv  # noqa: E402

NUM_BASES = 30
# (name, Cin or None = the featureless layer (Cin = N), Cout)
WORKLOADS = [("rgcn_conv1_featureless", None, 16), ("rgcn_conv2", 16, 2), ("rgcn_64_64", 64, 64)]


def example_graph(n_nodes, dev):
    spec = importlib.util.spec_from_file_location("example_rgcn", os.path.join(_ROOT, "examples", "rgcn.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ei, et = mod.entity_graph(n_nodes, 0)[:2]
    return ei.to(dev), et.to(dev), mod.NUM_RELATIONS


def upstream(conv, x, edge_index, edge_type):
    """PyG 1.4.3's RGCNConv in plain torch device ops."""
    src, dst = edge_index[0], edge_index[1]
    w = torch.matmul(conv.att, conv.basis.view(conv.num_bases, -1))
    if x is None:
        msg = torch.index_select(w.view(-1, conv.out_channels), 0, edge_type * conv.in_channels + src)
        n = conv.in_channels
    else:
        w = torch.index_select(w.view(conv.num_relations, conv.in_channels, conv.out_channels), 0, edge_type)
        msg = torch.bmm(x[src].unsqueeze(1), w).squeeze(-2)
        n = x.shape[0]
    out = torch.zeros(n, conv.out_channels, device=msg.device).index_add_(0, dst, msg)
    out = out + (conv.root if x is None else torch.matmul(x, conv.root))
    return out + conv.bias


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
    ap.add_argument("--nodes", type=int, default=23644)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    _lib.load()
    only = set(args.only.split(",")) if args.only else None
    n = args.nodes
    ei, et, n_rel = example_graph(n, dev)
    e = ei.shape[1]
    records = []
    for name, c_in, c_out in WORKLOADS:
        if only and name not in only:
            continue
        torch.manual_seed(0)
        featureless = c_in is None
        conv = RGCNConv(n if featureless else c_in, c_out, n_rel, NUM_BASES).to(dev)
        x = None if featureless else torch.randn(n, c_in, device=dev, requires_grad=True)
        picked = "gather (basis in place)" if featureless else ops.rgcn_form(NUM_BASES, c_in, c_out, e, n)
        variants = {"upstream": lambda: upstream(conv, x, ei, et),
                    "generic": lambda: conv.propagate(ei, size=(n, n), x=x, edge_type=et, edge_norm=None),
                    "picked": lambda: conv(x, ei, et)}
        if not featureless:
            variants["bins"] = lambda: conv(x, ei, et, form="bins")
            variants["gather"] = lambda: conv(x, ei, et, form="gather")

        def make_steps(fn):
            def fwd():
                with torch.no_grad():
                    fn()

            def train():
                conv.zero_grad(set_to_none=True)
                if x is not None:
                    x.grad = None
                fn().square().sum().backward()
            return fwd, train
        steps = {k: make_steps(v) for k, v in variants.items()}
        with torch.no_grad():
            ref = variants["upstream"]()
            diff = {k: float((variants[k]() - ref).abs().max()) for k in variants if k != "upstream"}
            scale = float(ref.abs().max())
        for fwd, train in steps.values():                              # warm-up (CSR builds, the plan, GEMM plans)
            for _ in range(3):
                fwd()
                train()
        torch.cuda.synchronize()
        times = {(k, p): [] for k in steps for p in ("fwd", "train")}
        for _ in range(args.repeats):
            for k, (fwd, train) in steps.items():
                times[(k, "fwd")].append(window_ms(fwd, args.window))
                times[(k, "train")].append(window_ms(train, args.window))
        rec = {"workload": name, "N": n, "E": e, "R": n_rel, "B": NUM_BASES, "Cin": n if featureless else c_in,
               "Cout": c_out, "featureless": featureless, "picked_form": picked, "max_abs_out": scale,
               "max_abs_diff_vs_upstream": diff, "source_hash": _lib.source_hash()}
        for (k, p), v in times.items():
            v = sorted(v)
            rec["%s_%s_ms" % (k, p)] = round(v[len(v) // 2], 4)
            rec["%s_%s_spread_ms" % (k, p)] = round(v[-1] - v[0], 4)
        for k, (_fwd, train) in steps.items():
            rec["%s_train_peak_bytes" % k] = peak_bytes(train)
        slack = rec["picked_train_spread_ms"] + rec["upstream_train_spread_ms"]
        rec["bar_met"] = rec["picked_train_ms"] <= rec["upstream_train_ms"] + slack
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
