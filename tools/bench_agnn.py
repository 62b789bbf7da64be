"""AGNNConv layer bench: the fused path (csrc/mp_agnn.hip) against this repository's
generic MessagePassing path (the layer's own message: native gathers of x_j /
x_norm_i / x_norm_j, utils.softmax on native segment ops, the native segmented
sum) and against upstream's recipe in torch device ops (F.normalize, index_select,
scatter max / sum softmax with the 1e-16, index_add_).  All three start from the
same looped edge list.

Shapes: the layer of examples/agnn.py (F = 16) on its Cora-shaped graph (2708
nodes), and a power-law graph of 100 k nodes and 1 M edges (mi355_mp.graphgen) at
F = 64 and F = 256.

Per variant: forward + backward of one layer with a learned beta (loss = sum of
squares, gradients for x and beta), timed with device events after a warm-up, in
windows of at least --window seconds, the variants alternating inside every
repeat (median and max - min over the repeats), and the peak device memory of one
forward + backward above what was allocated before it.  One JSON line per shape;
--out also writes them to a file with the native source hash.

    python tools/bench_agnn.py [--out profiles/agnn_bench.json]
"""
import argparse
import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mi355_mp import _lib  # noqa: E402
from mi355_mp.graphgen import cora_like, powerlaw_edge_index  # noqa: E402
from torch_geometric.nn import AGNNConv  # noqa: E402
from torch_geometric.nn.conv._structure import gat_loops  # noqa: E402

# (name, graph, F)
WORKLOADS = [("agnn_cora_f16", "cora", 16), ("agnn_100k_1m_f64", "large", 64), ("agnn_100k_1m_f256", "large", 256)]


def upstream(x, ei, beta):
    """PyG 1.4.3's AGNNConv message, softmax and aggregation in plain torch device ops."""
    src, dst = ei[0], ei[1]
    n = x.shape[0]
    xn = F.normalize(x, p=2, dim=-1)
    s = beta * (xn.index_select(0, dst) * xn.index_select(0, src)).sum(dim=-1)
    m = torch.full((n,), float("-inf"), device=x.device).scatter_reduce(0, dst, s.detach(), "amax")
    e = (s - m.index_select(0, dst)).exp()
    a = e / (torch.zeros(n, device=x.device).index_add_(0, dst, e).index_select(0, dst) + 1e-16)
    return torch.zeros_like(x).index_add_(0, dst, x.index_select(0, src) * a.view(-1, 1))


def generic(conv, x, ei):
    return conv.propagate(ei, x=x, x_norm=F.normalize(x, p=2, dim=-1), num_nodes=x.size(0))


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
    for name, which, width in WORKLOADS:
        if only and name not in only:
            continue
        if which not in graphs:
            graphs[which] = cora_like()["edge_index"].to(dev) if which == "cora" else \
                powerlaw_edge_index(100_000, 1_000_000, seed=3, device=dev)
        ei = graphs[which]
        n = 2708 if which == "cora" else 100_000
        torch.manual_seed(0)
        conv = AGNNConv(requires_grad=True).to(dev)
        x = torch.randn(n, width, device=dev, requires_grad=True)
        assert conv._fused_ok(x, ei)
        ei2 = gat_loops(ei, n)
        variants = {"upstream": lambda: upstream(x, ei2, conv.beta),
                    "generic": lambda: generic(conv, x, ei2),
                    "fused": lambda: conv(x, ei)}

        def make_step(fn):
            def train():
                conv.zero_grad(set_to_none=True)
                x.grad = None
                fn().square().sum().backward()
            return train
        steps = {k: make_step(v) for k, v in variants.items()}
        with torch.no_grad():
            ref = variants["upstream"]()
            diff = {k: float((variants[k]() - ref).abs().max()) for k in variants if k != "upstream"}
            scale = float(ref.abs().max())
        for train in steps.values():                                    # warm-up (loops, CSR builds)
            for _ in range(3):
                train()
        torch.cuda.synchronize()
        times = {k: [] for k in steps}
        for _ in range(args.repeats):
            for k, train in steps.items():
                times[k].append(window_ms(train, args.window))
        rec = {"workload": name, "N": n, "E": int(ei2.shape[1]), "F": width, "max_abs_out": scale,
               "max_abs_diff_vs_upstream": diff, "one_E_F_array_bytes": int(ei2.shape[1]) * width * 4,
               "source_hash": _lib.source_hash()}
        for k, v in times.items():
            v = sorted(v)
            rec["%s_train_ms" % k] = round(v[len(v) // 2], 4)
            rec["%s_train_spread_ms" % k] = round(v[-1] - v[0], 4)
        for k, train in steps.items():
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
