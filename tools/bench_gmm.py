"""GMMConv layer bench: the fused path (each forced form and the form the layer
picks) against upstream's recipe in torch device ops -- (x g).view(N, K, M)
gathered per edge into [E, K, M], the [E, K, D] and [E, K] Gaussian
intermediates, multiply, sum over K, index_add_ -- and against this
repository's generic MessagePassing path (the same message, native gathers and
segmented reduce).

Shapes: the two layers of examples/mnist_gmm_conv.py on 64 superpixel-sized
graphs of 75 nodes (about 1400 directed edges each, as MNISTSuperpixels has),
and one larger graph of 131072 nodes and 1048576 edges at Cin = Cout = 64, K =
25, D = 3.

Per variant: forward alone (no autograd) and forward + backward of one layer
(loss = sum of squares, gradients for x and every parameter), timed with device
events after a warm-up, in windows of at least --window seconds, the variants
alternating inside every repeat (median and max - min over the repeats), and
the peak device memory of one forward + backward above what was allocated
before it.  One JSON line per shape; --out also writes them to a file with the
native source hash.  The bar: the layer's pick is not slower forward + backward
than the upstream recipe by more than the two spreads together.

    python tools/bench_gmm.py [--out profiles/gmm_bench.json]
"""
import argparse
import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402

from mi355_mp import _lib, ops  # noqa: E402
from torch_geometric.nn import GMMConv  # noqa: E402

# (name, graphs, nodes per graph, edges per graph, D, K, Cin, Cout, aggr)
WORKLOADS = [
    ("mnist_conv1", 64, 75, 1400, 2, 25, 1, 32, "mean"),
    ("mnist_conv2", 64, 75, 1400, 2, 25, 32, 64, "mean"),
    ("large", 1024, 128, 1024, 3, 25, 64, 64, "mean"),
]


def make_graph(graphs, block, per_graph, seed, dev):
    """per_graph random edges inside each block of `block` nodes (a batch of small graphs)."""
    g = torch.Generator().manual_seed(seed)
    e = graphs * per_graph
    dst = torch.randint(0, graphs * block, (e,), generator=g)
    src = dst // block * block + torch.randint(0, block, (e,), generator=g)
    return torch.stack([src, dst]).to(dev)


def upstream(conv, x, edge_index, pseudo):
    """PyG 1.4.3's GMMConv (shared Gaussians) in plain torch device ops."""
    src, dst = edge_index[0], edge_index[1]
    K, M, D = conv.kernel_size, conv.out_channels, conv.dim
    y = torch.matmul(x, conv.g)[src].view(-1, K, M)
    gaussian = -0.5 * (pseudo.view(-1, 1, D) - conv.mu.view(1, K, D)).pow(2)
    gaussian = gaussian / (1e-15 + conv.sigma.view(1, K, D).pow(2))
    gaussian = torch.exp(gaussian.sum(dim=-1))
    msg = (y * gaussian.view(-1, K, 1)).sum(dim=-2)
    out = torch.zeros(x.shape[0], M, device=x.device).index_add_(0, dst, msg)
    if conv.aggr == "mean":
        deg = torch.zeros(x.shape[0], device=x.device).index_add_(0, dst, torch.ones_like(dst, dtype=torch.float32))
        out = out / deg.clamp(min=1).view(-1, 1)
    if conv.root is not None:
        out = out + torch.mm(x, conv.root)
    return out + conv.bias


def generic(conv, x, edge_index, pseudo):
    """The layer's own generic branch: upstream's message on the MessagePassing path."""
    out = conv.propagate(edge_index, x=torch.matmul(x, conv.g), pseudo=pseudo)
    if conv.root is not None:
        out = out + torch.matmul(x, conv.root)
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
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    _lib.load()
    only = set(args.only.split(",")) if args.only else None
    records = []
    for name, graphs, block, per_graph, D, K, c_in, c_out, aggr in WORKLOADS:
        if only and name not in only:
            continue
        n, e = graphs * block, graphs * per_graph
        ei = make_graph(graphs, block, per_graph, 1, dev)
        pseudo = torch.rand(e, D, generator=torch.Generator().manual_seed(2)).to(dev)
        torch.manual_seed(0)
        conv = GMMConv(c_in, c_out, D, K, aggr=aggr).to(dev)
        with torch.no_grad():                                          # Gaussians spread over the unit cube
            conv.mu.uniform_(0, 1)
            conv.sigma.uniform_(0.25, 0.75)
        x = torch.randn(n, c_in, device=dev, requires_grad=True)
        picked = ops.gmm_form(K, D, c_in, c_out, e, n)
        variants = {"upstream": lambda: upstream(conv, x, ei, pseudo),
                    "generic": lambda: generic(conv, x, ei, pseudo),
                    "bins": lambda: conv(x, ei, pseudo, form="bins"),
                    "gather": lambda: conv(x, ei, pseudo, form="gather"),
                    "picked": lambda: conv(x, ei, pseudo)}

        def make_steps(fn):
            def fwd():
                with torch.no_grad():
                    fn()

            def train():
                conv.zero_grad(set_to_none=True)
                x.grad = None
                fn().square().sum().backward()
            return fwd, train
        steps = {k: make_steps(v) for k, v in variants.items()}
        with torch.no_grad():
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
        rec = {"workload": name, "N": n, "E": e, "K": K, "D": D, "Cin": c_in, "Cout": c_out, "aggr": aggr,
               "picked_form": picked, "max_abs_out": scale, "max_abs_diff_vs_upstream": diff,
               "source_hash": _lib.source_hash()}
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
        del conv, x, ei, pseudo
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0),
                       "window_s": args.window, "repeats": args.repeats, "records": records}, fh, indent=1)
            fh.write("\n")
    return records


if __name__ == "__main__":
    main()
