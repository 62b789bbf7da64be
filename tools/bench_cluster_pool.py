"""Cluster-pooling stage bench: one voxel_grid + max_pool stage of the native
layer against the upstream recipe written in torch device ops (PyG 1.4.3's
chain: the voxel arithmetic, a unique of the cluster vector, scatter_reduce
amax and the second pass for its argmax, index_add_ means, a scatter_ for perm,
the relabelled edges with a boolean-mask self-loop removal, then torch_sparse's
coalesce as a sort, a second unique and an index_add_).  The parent of this
layer had no cluster pooling at all, so the composition is the yardstick.

Forward only (no autograd), timed with device events after a warm-up, in windows
of at least --window seconds, the two variants alternating inside every repeat;
then the native stage's steps one by one (each with its own window).  Two
shapes: the example's batch (64 graphs x 75 nodes, 8 neighbours, F = 32, 5-wide
voxels on [0, 28)^2) and a large one (2^20 nodes, 2^23 edges, F = 64).  One JSON
line per shape; --out also writes them to a file with the native source hash;
--dump-outputs DIR saves what the native stage computed (x, pos, batch,
edge_index, edge_attr as .npy) for a comparison across builds.

    python tools/bench_cluster_pool.py [--out profiles/cluster_pool_bench.json]
"""
import argparse
import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))

import torch  # noqa: E402

from mi355_mp import _lib, ops  # noqa: E402
from torch_geometric.data import Batch  # noqa: E402
from torch_geometric.nn import max_pool, voxel_grid  # noqa: E402


def example_batch(seed, dev, graphs=64, nodes=75, neighbours=8, F=32):
    """The example's first stage: `graphs` point sets on [0, 28)^2, every node linked
    to its nearest neighbours."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(graphs, nodes, 2, generator=g) * 28
    d = torch.cdist(pos, pos)
    d.diagonal(dim1=1, dim2=2).fill_(float("inf"))
    nbr = d.topk(neighbours, largest=False).indices + (torch.arange(graphs) * nodes).view(-1, 1, 1)
    dst = torch.arange(graphs * nodes).view(-1, 1).expand(-1, neighbours).reshape(-1)
    ei = torch.stack([nbr.reshape(-1), dst])
    n = graphs * nodes
    batch = torch.arange(graphs).repeat_interleave(nodes)
    x = torch.randn(n, F, generator=g)
    attr = torch.rand(ei.size(1), 2, generator=g)
    return {"x": x.to(dev), "pos": pos.view(n, 2).to(dev), "batch": batch.to(dev), "edge_index": ei.to(dev),
            "edge_attr": attr.to(dev), "size": 5.0, "start": 0.0, "end": 28.0}


def large_graph(seed, dev, n=1 << 20, deg=8, F=64, side=1024.0, size=2.0):
    """One graph of n points on [0, side)^2, stored row by row of 2-wide voxels so that
    index neighbours are spatial neighbours; every node links to `deg` nodes at most
    32 positions away (loops and duplicate cluster pairs are common)."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(n, 2, generator=g) * side
    order = ((pos[:, 1] / size).long() * int(side / size) + (pos[:, 0] / size).long()).argsort()
    pos = pos[order].contiguous()
    dst = torch.arange(n).repeat_interleave(deg)
    src = (dst + torch.randint(-32, 33, (n * deg,), generator=g)).clamp(0, n - 1)
    x = torch.randn(n, F, generator=g)
    attr = torch.rand(n * deg, 2, generator=g)
    return {"x": x.to(dev), "pos": pos.to(dev), "batch": torch.zeros(n, dtype=torch.int64, device=dev),
            "edge_index": torch.stack([src, dst]).to(dev), "edge_attr": attr.to(dev), "size": size, "start": 0.0,
            "end": side}


WORKLOADS = [("example_64x75_k8_F32", lambda dev: example_batch(1, dev)),
             ("large_2e20_nodes_2e23_edges_F64", lambda dev: large_graph(2, dev))]


def native_stage(w):
    cluster = voxel_grid(w["pos"], w["batch"], w["size"], w["start"], w["end"])
    return max_pool(cluster, Batch(batch=w["batch"], x=w["x"], pos=w["pos"], edge_index=w["edge_index"],
                                   edge_attr=w["edge_attr"]))


def upstream_stage(w):
    """The same stage as upstream runs it, in torch device ops."""
    x, pos, batch, ei, attr = w["x"], w["pos"], w["batch"], w["edge_index"], w["edge_attr"]
    n = x.size(0)
    dev = x.device
    # voxel_grid / grid_cluster
    p = torch.cat([pos, batch.unsqueeze(-1).to(pos.dtype)], dim=-1)
    size = torch.tensor([w["size"], w["size"], 1.0], device=dev)
    start = torch.tensor([w["start"], w["start"], 0.0], device=dev)
    end = torch.cat([torch.tensor([w["end"], w["end"]], device=dev), batch.max().to(pos.dtype).view(1)])
    c = ((p - start) / size).long()
    m = ((end - start) / size).long() + 1
    mult = torch.cat([m.new_ones(1), m.cumprod(0)[:-1]])
    cluster = (c * mult).sum(1)
    # consecutive_cluster
    uniq, inv = torch.unique(cluster, sorted=True, return_inverse=True)
    M = uniq.numel()
    perm = inv.new_empty(M).scatter_(0, inv, torch.arange(n, device=dev))
    # scatter_('max'): the maximum, then the pass that finds its argument, then the mask
    idx = inv.view(-1, 1).expand_as(x)
    out = x.new_full((M, x.size(1)), torch.finfo(x.dtype).min).scatter_reduce_(0, idx, x, "amax", include_self=True)
    rows = torch.arange(n, device=dev).view(-1, 1).expand_as(x)
    arg = rows.new_full(out.shape, n).scatter_reduce_(0, idx, torch.where(x == out[inv], rows, n), "amin",
                                                      include_self=True)
    out = out.masked_fill(out < -10000, 0.0)
    # scatter_mean of the positions
    cnt = pos.new_zeros(M).index_add_(0, inv, pos.new_ones(n)).clamp_(min=1)
    pos_out = pos.new_zeros((M, pos.size(1))).index_add_(0, inv, pos) / cnt.view(-1, 1)
    batch_out = batch[perm]
    # pool_edge: relabel, remove_self_loops, coalesce
    e = inv[ei.view(-1)].view(2, -1)
    mask = e[0] != e[1]
    e, a = e[:, mask], attr[mask]
    if e.numel() > 0:
        key, order = (e[0] * M + e[1]).sort()
        a = a[order]
        uk, inv2 = torch.unique(key, sorted=True, return_inverse=True)
        e = torch.stack([uk // M, uk % M])
        a = a.new_zeros((uk.numel(),) + tuple(a.shape[1:])).index_add_(0, inv2, a)
    return Batch(batch=batch_out, x=out, pos=pos_out, edge_index=e, edge_attr=a), arg


def native_steps(w):
    """The native stage's steps as separate callables over fixed inputs (the step
    before each has run once), for the per-step split."""
    dev = w["x"].device
    geo = [torch.tensor([w[k], w[k], v], device=dev) for k, v in (("size", 1.0), ("start", 0.0))]
    geo.append(torch.cat([torch.tensor([w["end"], w["end"]], device=dev), w["batch"].max().float().view(1)]))
    key = ops.voxel_keys(w["pos"], w["batch"], *geo)
    sel = ops.cluster_build(key)
    ep = ops.pool_edges(w["edge_index"], sel)
    return {"voxel_keys": lambda: ops.voxel_keys(w["pos"], w["batch"], *geo),
            "cluster_build": lambda: ops.cluster_build(key),
            "cluster_reduce": lambda: ops.cluster_reduce(sel, w["x"], "max", pos=w["pos"], batch=w["batch"]),
            "pool_edges": lambda: ops.pool_edges(w["edge_index"], sel),
            "pool_edge_attr": lambda: ops.pool_edge_attr_sum(w["edge_attr"], ep, sel),
            "read_counts": lambda: sel.counts.tolist()}


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


def dump(dirname, name, out):
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    for k in ("x", "pos", "batch", "edge_index", "edge_attr"):
        np.save(os.path.join(dirname, "%s_%s.npy" % (name, k)), out[k].detach().cpu().numpy())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    ap.add_argument("--out", default=None)
    ap.add_argument("--dump-outputs", default="", metavar="DIR")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    _lib.load()
    only = set(args.only.split(",")) if args.only else None
    records = []
    for name, build in WORKLOADS:
        if only and name not in only:
            continue
        w = build(dev)
        steps = {"native": lambda: native_stage(w), "upstream_torch_ops": lambda: upstream_stage(w)}
        with torch.no_grad():
            a, (b, _) = native_stage(w), upstream_stage(w)
            same_index = bool(a.edge_index.shape == b.edge_index.shape and torch.equal(a.edge_index, b.edge_index))
            same_x = bool(a.x.shape == b.x.shape and torch.equal(a.x, b.x))
            same_batch = bool(torch.equal(a.batch, b.batch))
            pos_err = float((a.pos - b.pos).abs().max())
            attr_err = float((a.edge_attr - b.edge_attr).abs().max()) if same_index and a.edge_attr.numel() else None
            if args.dump_outputs:
                dump(args.dump_outputs, name, a)
            split = native_steps(w)
            for s in list(steps.values()) + list(split.values()):
                for _ in range(3):
                    s()
            torch.cuda.synchronize()
            times = {k: [] for k in steps}
            for _ in range(args.repeats):
                for k, s in steps.items():
                    times[k].append(window_ms(s, args.window))
            split_ms = {k: round(window_ms(s, args.window / 4), 4) for k, s in split.items()}
        rec = {"workload": name, "N": int(w["x"].size(0)), "E": int(w["edge_index"].size(1)), "F": int(w["x"].size(1)),
               "clusters": int(a.x.size(0)), "edges_out": int(a.edge_index.size(1)),
               "same_x_as_upstream": same_x, "same_edge_index_as_upstream": same_index,
               "same_batch_as_upstream": same_batch, "pos_max_abs_diff": pos_err, "edge_attr_max_abs_diff": attr_err,
               "native_steps_ms": split_ms, "source_hash": _lib.source_hash()}
        for k, v in times.items():
            v = sorted(v)
            rec[k + "_ms"] = round(v[len(v) // 2], 4)
            rec[k + "_spread_ms"] = round(v[-1] - v[0], 4)
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del w, a, b, split, steps
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0),
                       "window_s": args.window, "repeats": args.repeats, "records": records}, fh, indent=1)
            fh.write("\n")
    return records


if __name__ == "__main__":
    main()
