"""Dense family bench: dense_diff_pool forward + backward and one DenseSAGEConv
(forward + backward), each as the fused native call (csrc/mp_dense.hip) and as
the upstream recipe in torch device ops, with the peak device memory of a step.

Shapes: the DiffPool example's first level (B = 20, N = 100, C = 10, F = 192:
one workgroup per graph) and one beyond it (B = 32, N = 1000, C = 100, F = 64:
row tiles).  adj is 0/1 data adjacency without a gradient, as at a first level.

The record also names what the layers pick at the shape (nn/dense/_dense.py).

Per variant a training step (loss = sum of the outputs' squares plus the two
losses; gradients for x and s, or x and the layer's parameters) and the forward
alone, timed with device events after a warm-up in windows of at least --window
seconds, the variants alternating inside every repeat (median and max - min over
the repeats).  One JSON line per shape; --out also writes them to a file with
the native source hash.

    python tools/bench_dense.py [--out profiles/dense_bench.json]
"""
import argparse
import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402

from mi355_mp import _lib, ops  # noqa: E402
from torch_geometric.nn import DenseSAGEConv  # noqa: E402
from torch_geometric.nn.dense import _dense  # noqa: E402

WORKLOADS = {"example_b20_n100_c10_f192": (20, 100, 10, 192), "tiles_b32_n1000_c100_f64": (32, 1000, 100, 64)}


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


def peak_mib(step):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    _lib.load()
    only = set(args.only.split(",")) if args.only else None
    records = []
    for name, (B, N, C, F) in WORKLOADS.items():
        if only and name not in only:
            continue
        g = torch.Generator().manual_seed(5)
        adj = (torch.rand(B, N, N, generator=g) < 0.05).float()
        adj = torch.maximum(adj, adj.transpose(1, 2)).to(dev)
        mask = (torch.arange(N).view(1, N) < torch.randint(N // 2, N + 1, (B, 1), generator=g)).to(dev)
        x = torch.randn(B, N, F, generator=g).to(dev).requires_grad_(True)
        s = torch.randn(B, N, C, generator=g).to(dev).requires_grad_(True)
        torch.manual_seed(0)
        conv = DenseSAGEConv(F, C).to(dev)

        def pool_loss(res):
            out, out_adj, link, ent = res
            return out.square().sum() + out_adj.square().sum() + link + ent

        def conv_with(agg):
            h = torch.matmul(agg(x, adj, True), conv.weight) + conv.bias
            return h * mask.view(B, N, 1).to(h.dtype)

        variants = {"pool_fused": lambda: pool_loss(ops.dense_diff_pool(x, adj, s, mask)),
                    "pool_recipe": lambda: pool_loss(_dense.diff_pool_recipe(x, adj, s, mask)),
                    "sage_fused": lambda: conv_with(ops.dense_mean_agg).square().sum(),
                    "sage_recipe": lambda: conv_with(_dense.mean_agg_recipe).square().sum()}

        def make_steps(fn):
            def fwd():
                with torch.no_grad():
                    fn()

            def train():
                conv.zero_grad(set_to_none=True)
                x.grad = None
                s.grad = None
                fn().backward()
            return fwd, train
        run = {k: make_steps(v) for k, v in variants.items()}
        with torch.no_grad():
            a, b = ops.dense_diff_pool(x, adj, s, mask), _dense.diff_pool_recipe(x, adj, s, mask)
            diff = {"pool": max(float(((u - v).abs() / v.abs().clamp(min=1)).max()) for u, v in zip(a, b)),
                    "sage": float((conv_with(ops.dense_mean_agg) - conv_with(_dense.mean_agg_recipe)).abs().max())}
        for fwd, train in run.values():                                # warm-up
            for _ in range(3):
                fwd()
                train()
        torch.cuda.synchronize()
        times = {(k, p): [] for k in run for p in ("fwd", "train")}
        for _ in range(args.repeats):
            for k, (fwd, train) in run.items():
                times[(k, "fwd")].append(window_ms(fwd, args.window))
                times[(k, "train")].append(window_ms(train, args.window))
        rec = {"workload": name, "B": B, "N": N, "C": C, "F": F, "path": ops.diff_pool_path(N, C, F),
               "max_rel_diff_fused_vs_recipe": diff, "source_hash": _lib.source_hash()}
        for (k, p), v in times.items():
            v = sorted(v)
            rec["%s_%s_ms" % (k, p)] = round(v[len(v) // 2], 4)
            rec["%s_%s_spread_ms" % (k, p)] = round(v[-1] - v[0], 4)
        for k, (fwd, train) in run.items():
            rec["%s_train_peak_MiB" % k] = peak_mib(train)
        for fam in ("pool", "sage"):
            for p in ("fwd", "train"):
                slack = rec["%s_fused_%s_spread_ms" % (fam, p)] + rec["%s_recipe_%s_spread_ms" % (fam, p)]
                rec["%s_fused_not_slower_%s" % (fam, p)] = \
                    rec["%s_fused_%s_ms" % (fam, p)] <= rec["%s_recipe_%s_ms" % (fam, p)] + slack
                rec["%s_%s_recipe_over_fused" % (fam, p)] = round(
                    rec["%s_recipe_%s_ms" % (fam, p)] / rec["%s_fused_%s_ms" % (fam, p)], 2)
        # what the layers run at this shape (nn/dense/_dense.py), and whether that is the faster of the two
        for fam, pick in (("pool", _dense.pool_fused(x, adj, s)), ("sage", _dense.agg_fused(x, adj))):
            rec["%s_layer_pick" % fam] = "fused" if pick else "recipe"
            rec["%s_layer_pick_not_slower_train" % fam] = bool(not pick or rec["%s_fused_not_slower_train" % fam])
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del x, s, adj, mask, conv
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0),
                       "window_s": args.window, "repeats": args.repeats, "records": records}, fh, indent=1)
            fh.write("\n")
    return records


if __name__ == "__main__":
    main()
