"""TopKPooling layer bench: the native layer against the upstream recipe written
in torch device ops (PyG 1.4.3's chain: projection and tanh, a dense
[G, max_nodes] padded copy of the scores, one descending sort per row, a Python
loop building one arange per graph, x[perm] * score[perm], a -1-filled relabel
table and boolean-mask gathers over the edges).  The parent of this layer had no
pooling at all, so the composition is the yardstick.

Forward + backward of one TopKPooling(128, ratio=0.8) (loss = sum of squares of
x_out plus the sum of score[perm]), timed with device events after a warm-up,
in windows of at least --window seconds, the variants alternating inside every
repeat.  The native layer also runs with the workgroup limit
(MP_TUNE_TOPK_WG_LIMIT) halved and doubled.  One JSON line per shape; --out
also writes them to a file with the native source hash.

    python tools/bench_pool.py [--out profiles/topk_pool_bench.json]
"""
import argparse
import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402

from mi355_mp import _lib  # noqa: E402
from torch_geometric.nn import TopKPooling  # noqa: E402

F, RATIO = 128, 0.8


def small_graphs(seed, dev, n_graphs=1024, lo=2, hi=126, deg=4):
    """A batch of n_graphs graphs of lo..hi nodes with deg edges per node, both
    ends inside the graph."""
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(lo, hi + 1, (n_graphs,), generator=g)
    batch = torch.repeat_interleave(torch.arange(n_graphs), sizes)
    first = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)[:-1]])
    n = int(sizes.sum())
    dst = torch.arange(n).repeat_interleave(deg)
    src = first[batch[dst]] + (torch.rand(n * deg, generator=g) * sizes[batch[dst]]).long()
    return n, torch.stack([src, dst]).to(dev), batch.to(dev)


def one_graph(seed, dev, n=1 << 20, e=1 << 24):
    g = torch.Generator().manual_seed(seed)
    return n, torch.randint(0, n, (2, e), generator=g).to(dev), None


# (name, builder, the workgroup limits to try)
WORKLOADS = [
    ("batch_1024_graphs_2_126", lambda dev: small_graphs(1, dev), (1024, 2048, 4096)),
    ("batch_64_graphs_1500_3000", lambda dev: small_graphs(2, dev, 64, 1500, 3000), (1024, 2048, 4096)),
    ("one_graph_2e20_nodes_2e24_edges", lambda dev: one_graph(3, dev), (2048,)),
]


def upstream_topk(score, ratio, batch):
    n_graphs = int(batch.max()) + 1
    sizes = torch.bincount(batch, minlength=n_graphs)
    width = int(sizes.max())
    first = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)[:-1]])
    slot = torch.arange(batch.numel(), device=score.device) - first[batch] + batch * width
    dense = score.new_full((n_graphs * width,), torch.finfo(score.dtype).min)
    dense[slot] = score
    order = dense.view(n_graphs, width).sort(dim=-1, descending=True)[1] + first.view(-1, 1)
    order = order.view(-1)
    k = (ratio * sizes.to(torch.float)).ceil().to(torch.long)
    take = torch.cat([torch.arange(int(k[i]), device=score.device) + i * width for i in range(n_graphs)])
    return order[take]


def upstream_layer(x, edge_index, batch, weight, ratio):
    n = x.size(0)
    if batch is None:
        batch = edge_index.new_zeros(n)
    score = torch.tanh((x * weight).sum(dim=-1) / weight.norm(p=2, dim=-1))
    perm = upstream_topk(score, ratio, batch)
    x_out = x[perm] * score[perm].view(-1, 1)
    relabel = perm.new_full((n,), -1)
    relabel[perm] = torch.arange(perm.numel(), device=perm.device)
    row, col = relabel[edge_index[0]], relabel[edge_index[1]]
    keep = (row >= 0) & (col >= 0)
    return x_out, torch.stack([row[keep], col[keep]]), None, batch[perm], perm, score[perm]


def window_ms(step, min_s):
    """Mean ms per step over one window of at least min_s seconds (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, total = 0, 0.0
    reps = 1
    while total < min_s * 1e3:
        a.record()
        for _ in range(reps):
            step()
        b.record()
        b.synchronize()
        total += a.elapsed_time(b)
        n += reps
        reps = min(reps * 2, 64)
    return total / n


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    key = _lib.MP_TUNE_TOPK_WG_LIMIT
    default_limit = int(lib.mp_tune(key, -1))
    only = set(args.only.split(",")) if args.only else None
    records = []
    for name, build, limits in WORKLOADS:
        if only and name not in only:
            continue
        n, ei, batch = build(dev)
        torch.manual_seed(0)
        pool = TopKPooling(F, ratio=RATIO).to(dev)
        x = torch.relu(torch.randn(n, F, device=dev)).requires_grad_(True)

        def loss_of(out):
            return out[0].square().sum() + out[5].sum()

        def native(limit):
            def step():
                prev = lib.mp_tune(key, limit)
                try:
                    pool.zero_grad(set_to_none=True)
                    x.grad = None
                    loss_of(pool(x, ei, None, batch)).backward()
                finally:
                    lib.mp_tune(key, prev)
            return step

        def upstream():
            pool.zero_grad(set_to_none=True)
            x.grad = None
            loss_of(upstream_layer(x, ei, batch, pool.weight, RATIO)).backward()

        steps = {"native_L%d" % v: native(v) for v in limits}
        steps["upstream_torch_ops"] = upstream
        with torch.no_grad():
            a, b = pool(x, ei, None, batch), upstream_layer(x, ei, batch, pool.weight, RATIO)
            same_nodes = bool(a[4].numel() == b[4].numel())
            same_perm = same_nodes and bool(torch.equal(a[4], b[4]))       # ties may order differently upstream
            kept_nodes, kept_edges = int(a[4].numel()), int(a[1].shape[1])
            same_edges = bool(a[1].shape == b[1].shape)
        for s in steps.values():
            for _ in range(3):
                s()
        torch.cuda.synchronize()
        times = {k: [] for k in steps}
        for _ in range(args.repeats):
            for k, s in steps.items():
                times[k].append(window_ms(s, args.window))
        rec = {"workload": name, "N": n, "E": int(ei.shape[1]), "graphs": 1 if batch is None else int(batch[-1]) + 1,
               "F": F, "ratio": RATIO, "kept_nodes": kept_nodes, "kept_edges": kept_edges,
               "same_node_count_as_upstream": same_nodes, "same_perm_as_upstream": same_perm,
               "same_edge_count_as_upstream": same_edges, "default_limit": default_limit,
               "source_hash": _lib.source_hash()}
        for k, v in times.items():
            v = sorted(v)
            rec[k + "_ms"] = round(v[len(v) // 2], 4)
            rec[k + "_spread_ms"] = round(v[-1] - v[0], 4)
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del pool, x, ei, batch
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0),
                       "window_s": args.window, "repeats": args.repeats, "records": records}, fh, indent=1)
            fh.write("\n")
    return records


if __name__ == "__main__":
    main()
