"""One GatedGraphConv layer (L = 3 steps, sum aggregation) at C = 64 and 128,
forward and forward + backward, on the Cora-shaped graph of
examples/gated_graph.py and on a 100k-node / 1M-edge power-law graph:

  fused     the layer's fused path: the engine's aggregation of the state plus
            the one-kernel GRU cell (mi355_mp.ops.gru_cell, csrc/mp_gru.hip)
  recipe    upstream's forward in torch device ops (GatedGraphConv.recipe)

and the cell alone on the same node counts: the fused kernel (with the weight
image packed per call, as the layer does) against torch.nn.GRUCell.  Timed with
device events after a warm-up, in windows of at least --window seconds, the
variants alternating inside every repeat (median and max - min over the
repeats); the peak device memory of one forward + backward is recorded.

    python tools/bench_ggc.py [--out profiles/ggc_bench.json]
"""
import argparse
import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402

from mi355_mp import _lib, ops  # noqa: E402
from mi355_mp.graphgen import cora_like, powerlaw_edge_index  # noqa: E402
from torch_geometric.nn import GatedGraphConv  # noqa: E402

L = 3
WORKLOADS = [("ggc_cora", None), ("ggc_100k_1m", (100_000, 1_000_000))]


def window_ms(step, min_s):
    """Mean ms per step over one window of at least min_s seconds (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, total, batch = 0, 0.0, 1
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


def make_steps(module, fn):
    def fwd():
        with torch.no_grad():
            return fn()

    def train():
        module.zero_grad(set_to_none=True)
        fn().square().sum().backward()
    return fwd, train


def measure(steps, args):
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
    rec = {}
    for (k, p), v in times.items():
        v = sorted(v)
        rec["%s_%s_ms" % (k, p)] = round(v[len(v) // 2], 4)
        rec["%s_%s_spread_ms" % (k, p)] = round(v[-1] - v[0], 4)
    for k, (_fwd, train) in steps.items():
        rec["%s_train_peak_bytes" % k] = peak_bytes(train)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    _lib.load()
    records = []
    for name, which in WORKLOADS:
        if which is None:
            ei = cora_like()["edge_index"].to(dev)
            n = int(ei.max()) + 1
        else:
            ei = powerlaw_edge_index(which[0], which[1], seed=3, device=dev)
            n = which[0]
        for C in (64, 128):
            torch.manual_seed(0)
            x = torch.randn(n, C, device=dev)
            conv = GatedGraphConv(C, L).to(dev)
            assert conv.fused(x)
            steps = {"fused": make_steps(conv, lambda: conv(x, ei, form="fused")),
                     "recipe": make_steps(conv, lambda: conv(x, ei, form="unfused"))}
            diff = float((steps["fused"][0]() - steps["recipe"][0]()).abs().max())
            rec = {"workload": name, "what": "layer", "N": n, "E": int(ei.shape[1]), "C": C, "L": L,
                   "max_abs_diff_vs_recipe": diff}
            rec.update(measure(steps, args))
            print(json.dumps(rec), flush=True)
            records.append(rec)
            # the cell alone: a, h and the layer's own GRU parameters
            rnn = conv.rnn
            a = torch.randn(n, C, device=dev, requires_grad=True)
            h = torch.randn(n, C, device=dev, requires_grad=True)
            cell = {"fused": make_steps(rnn, lambda: ops.gru_cell(a, h, rnn.weight_ih.t(), rnn.weight_hh.t(),
                                                                  rnn.bias_ih, rnn.bias_hh)),
                    "grucell": make_steps(rnn, lambda: rnn(a, h))}
            diff = float((cell["fused"][0]() - cell["grucell"][0]()).abs().max())
            rec = {"workload": name, "what": "cell", "N": n, "C": C, "max_abs_diff_vs_grucell": diff}
            rec.update(measure(cell, args))
            print(json.dumps(rec), flush=True)
            records.append(rec)
            del conv, x, a, h
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0),
                       "window_s": args.window, "repeats": args.repeats, "records": records}, fh, indent=1)
            fh.write("\n")
    return records


if __name__ == "__main__":
    main()
