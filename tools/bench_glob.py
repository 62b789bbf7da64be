"""Attention readout bench: one Set2Set step's readout (query mode: scores,
per-graph softmax, weighted sum, q_star = [q | r]) in three variants --
  upstream  the recipe in torch device ops (scatter_reduce amax, index_add_)
  native    the recipe on this repository's softmax and scatter_ ops
  fused     ops.attention_readout (csrc/mp_glob.hip), one call
-- and the whole Set2Set layer (LSTM included) with the fused call and with the
native recipe.

Shapes: QM9 (128 graphs of 3 to 29 nodes, C = 64, 3 steps), ENZYMES-like (128
graphs of about 33 nodes, C = 128), 32 graphs of 4096 nodes (C = 64) and one
graph of 2^17 nodes (C = 64, the split path).

Per variant: forward alone (no autograd) and forward + backward (loss = sum of
squares; gradients for x and q, or x and the LSTM), timed with device events
after a warm-up in windows of at least --window seconds, the variants
alternating inside every repeat (median and max - min over the repeats).  For
the two large shapes the fused forward's achieved bytes per second against its
minimum traffic (N * C * 4 read + N * 4 written).  One JSON line per shape;
--out also writes them to a file with the native source hash.

    python tools/bench_glob.py [--out profiles/glob_bench.json]
"""
import argparse
import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402

from mi355_mp import _lib, ops  # noqa: E402
from torch_geometric.nn import Set2Set  # noqa: E402
from torch_geometric.nn.glob import _readout  # noqa: E402


def sizes_of(name):
    g = torch.Generator().manual_seed(3)
    if name == "qm9":
        return torch.randint(3, 30, (128,), generator=g).tolist(), 64, 3
    if name == "enzymes":
        return torch.randint(25, 42, (128,), generator=g).tolist(), 128, 3
    if name == "g32_n4096":
        return [4096] * 32, 64, 3
    return [1 << 17], 64, 3


WORKLOADS = ["qm9", "enzymes", "g32_n4096", "g1_n131072"]


def upstream(x, q, batch, G):
    e = (x * q[batch]).sum(dim=-1, keepdim=True)
    m = torch.zeros((G, 1), device=x.device).scatter_reduce(0, batch.view(-1, 1), e.detach(), "amax",
                                                            include_self=False)
    p = (e - m[batch]).exp()
    a = p / (torch.zeros((G, 1), device=x.device).index_add_(0, batch, p)[batch] + 1e-16)
    r = torch.zeros((G, x.shape[1]), device=x.device).index_add_(0, batch, a * x)
    return torch.cat([q, r], dim=-1)


def native(x, q, batch, G):
    e = (x * q[batch]).sum(dim=-1, keepdim=True)
    return torch.cat([q, _readout.recipe(x, e, batch, G)], dim=-1)


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
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    _lib.load()
    only = set(args.only.split(",")) if args.only else None
    records = []
    for name in WORKLOADS:
        if only and name not in only:
            continue
        sizes, C, steps = sizes_of(name)
        G, n = len(sizes), sum(sizes)
        batch = torch.repeat_interleave(torch.arange(G), torch.tensor(sizes)).to(dev)
        layout = ops.cached_batch_layout(batch, n, dev)
        torch.manual_seed(0)
        x = torch.randn(n, C, device=dev, requires_grad=True)
        q = torch.randn(G, C, device=dev, requires_grad=True)
        layer = Set2Set(C, steps).to(dev)

        def layer_native():
            old = _readout.fused_layout
            _readout_set(lambda *a: None)
            try:
                return layer(x, batch)
            finally:
                _readout_set(old)

        variants = {"upstream": lambda: upstream(x, q, batch, G),
                    "native": lambda: native(x, q, batch, G),
                    "fused": lambda: ops.attention_readout(x, layout, q=q, out=x.new_empty(G, 2 * C), col=C),
                    "layer_native": layer_native,
                    "layer_fused": lambda: layer(x, batch)}

        def make_steps(fn):
            def fwd():
                with torch.no_grad():
                    fn()

            def train():
                layer.zero_grad(set_to_none=True)
                x.grad = None
                q.grad = None
                fn().square().sum().backward()
            return fwd, train
        run = {k: make_steps(v) for k, v in variants.items()}
        with torch.no_grad():
            ref = variants["upstream"]()
            diff = {k: float((variants[k]() - ref).abs().max()) for k in ("native", "fused")}
            diff["layer_fused_vs_layer_native"] = float((variants["layer_fused"]() - variants["layer_native"]()).abs().max())
        for fwd, train in run.values():                                # warm-up (CSR builds, LSTM plans)
            for _ in range(3):
                fwd()
                train()
        torch.cuda.synchronize()
        times = {(k, p): [] for k in run for p in ("fwd", "train")}
        for _ in range(args.repeats):
            for k, (fwd, train) in run.items():
                times[(k, "fwd")].append(window_ms(fwd, args.window))
                times[(k, "train")].append(window_ms(train, args.window))
        rec = {"workload": name, "graphs": G, "N": n, "C": C, "steps": steps,
               "paths": sorted({ops.readout_path(s, C) for s in sizes}), "max_abs_diff_vs_upstream": diff,
               "source_hash": _lib.source_hash()}
        for (k, p), v in times.items():
            v = sorted(v)
            rec["%s_%s_ms" % (k, p)] = round(v[len(v) // 2], 4)
            rec["%s_%s_spread_ms" % (k, p)] = round(v[-1] - v[0], 4)
        if n >= 1 << 17:
            rec["fused_fwd_min_traffic_GBps"] = round((n * C * 4 + n * 4) / (rec["fused_fwd_ms"] * 1e-3) / 1e9, 1)
        for p in ("fwd", "train"):
            for other in ("upstream", "native"):
                slack = rec["fused_%s_spread_ms" % p] + rec["%s_%s_spread_ms" % (other, p)]
                rec["fused_not_slower_than_%s_%s" % (other, p)] = \
                    rec["fused_%s_ms" % p] <= rec["%s_%s_ms" % (other, p)] + slack
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del x, q, batch, layer
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0),
                       "window_s": args.window, "repeats": args.repeats, "records": records}, fh, indent=1)
            fh.write("\n")
    return records


def _readout_set(fn):
    """Route the layers to the recipe (fn returns None) or back to the fused call."""
    from torch_geometric.nn.glob import attention, set2set
    _readout.fused_layout = fn
    set2set.fused_layout = fn
    attention.fused_layout = fn


if __name__ == "__main__":
    main()
