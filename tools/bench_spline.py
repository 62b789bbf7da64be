"""SplineConv layer bench: the fused path (each forced form and the automatic
one) against a composition that runs only the engine's existing aggregation
kernel -- the standalone basis, an edge list expanded S-fold with
col = j*K + wi and weight b (mean folded into the weight), then
fused_propagate over x @ W laid out [N*K, Fout].

Forward + backward of one layer (loss = sum of squares), timed with device
events after a warm-up, in windows of at least --window seconds, the variants
alternating inside every repeat.  The composition's expanded graph, its CSRs
and its weights are built once outside the timed region (reported as
prep_ms), which favours the composition: upstream recomputes the basis on
every forward.  One JSON line per shape; --out also writes them to a file with
the native source hash.

    python tools/bench_spline.py [--out profiles/spline_conv_bench.json]
"""
import argparse
import json
import os
import sys
import time

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402

from mi355_mp import _lib, ops  # noqa: E402
from mi355_mp.graph import Graph  # noqa: E402
from torch_geometric.nn import SplineConv  # noqa: E402

# (name, nodes, edges, D, kernel_size, [(Fin, Fout), ...], nodes per graph of a batch or None)
WORKLOADS = [
    ("superpixel_256", 256 * 75, 360000, 2, 5, [(1, 32), (32, 64)], 75),
    ("superpixel_4096", 4096 * 75, 5760000, 2, 5, [(1, 32), (32, 64)], 75),
    ("mesh", 6890, 41328, 3, 5, [(1, 32), (64, 64)], None),
    ("citation", 2708, 10556, 1, 2, [(1433, 16), (16, 7)], None),
]


def make_graph(n, e, block, seed, dev):
    """e random edges; block: both ends inside the same block of `block` nodes
    (a batch of small graphs)."""
    g = torch.Generator().manual_seed(seed)
    dst = torch.randint(0, n, (e,), generator=g)
    if block:
        src = dst // block * block + torch.randint(0, block, (e,), generator=g)
    else:
        src = torch.randint(0, n, (e,), generator=g)
    return torch.stack([src, dst]).to(dev)


class Composition(object):
    """The layer through the existing kernels only (see the module docstring)."""

    def __init__(self, conv, edge_index, pseudo, n):
        t0 = time.perf_counter()
        K = conv.weight.shape[0]
        b, wi = ops.spline_basis(pseudo, conv._kernel_size, conv._is_open_spline, conv.degree)
        S = b.shape[1]
        src, dst = edge_index[0], edge_index[1]
        deg = torch.bincount(dst, minlength=n).clamp(min=1).to(torch.float32)
        self.w = (b / deg[dst].view(-1, 1)).reshape(-1).contiguous()
        self.ei = torch.stack([(src.view(-1, 1) * K + wi).reshape(-1), dst.view(-1, 1).expand(-1, S).reshape(-1)])
        self.graph = Graph(self.ei, n, n * K)
        self.graph.dst, self.graph.src                                     # both CSRs built here
        torch.cuda.synchronize()
        self.prep_ms = (time.perf_counter() - t0) * 1e3
        self.conv, self.K, self.n = conv, K, n

    def __call__(self, x):
        c = self.conv
        f_in, f_out = c.weight.shape[1], c.weight.shape[2]
        xw = torch.matmul(x, c.weight.permute(1, 0, 2).reshape(f_in, self.K * f_out)).view(self.n * self.K, f_out)
        out = ops.fused_propagate(self.graph, xw, self.ei, edge_weight=self.w, reduce="sum")
        return out + torch.matmul(x, c.root) + c.bias


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    _lib.load()
    only = set(args.only.split(",")) if args.only else None
    records = []
    for name, n, e, D, ks, layers, block in WORKLOADS:
        if only and name not in only:
            continue
        ei = make_graph(n, e, block, 1, dev)
        pseudo = torch.rand(e, D, generator=torch.Generator().manual_seed(2)).to(dev)
        for f_in, f_out in layers:
            torch.manual_seed(0)
            conv = SplineConv(f_in, f_out, dim=D, kernel_size=ks).to(dev)
            x = torch.randn(n, f_in, device=dev, requires_grad=True)
            comp = Composition(conv, ei, pseudo, n)
            variants = {"bins": lambda: conv(x, ei, pseudo, form="bins"),
                        "gather": lambda: conv(x, ei, pseudo, form="gather"),
                        "auto": lambda: conv(x, ei, pseudo),
                        "composition": lambda: comp(x)}

            def make_step(fn):
                def step():
                    conv.zero_grad(set_to_none=True)
                    x.grad = None
                    fn().square().sum().backward()
                return step
            steps = {k: make_step(v) for k, v in variants.items()}
            with torch.no_grad():
                diff = float((variants["auto"]() - variants["composition"]()).abs().max())
            for s in steps.values():                                       # warm-up (CSR builds, GEMM plans)
                for _ in range(3):
                    s()
            torch.cuda.synchronize()
            times = {k: [] for k in steps}
            for _ in range(args.repeats):
                for k, s in steps.items():
                    times[k].append(window_ms(s, args.window))
            S = (conv.degree + 1) ** D
            rec = {"workload": name, "N": n, "E": e, "D": D, "kernel_size": ks, "Fin": f_in, "Fout": f_out,
                   "auto_form": ops.spline_form(S, f_in, f_out, conv.weight.shape[0]),
                   "max_abs_diff_vs_composition": diff,
                   "composition_prep_ms": round(comp.prep_ms, 3), "source_hash": _lib.source_hash()}
            for k, v in times.items():
                v = sorted(v)
                rec[k + "_ms"] = round(v[len(v) // 2], 4)
                rec[k + "_spread_ms"] = round(v[-1] - v[0], 4)
            print(json.dumps(rec), flush=True)
            records.append(rec)
            del comp, conv, x
        del ei, pseudo
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0),
                       "window_s": args.window, "repeats": args.repeats, "records": records}, fh, indent=1)
            fh.write("\n")
    return records


if __name__ == "__main__":
    main()
