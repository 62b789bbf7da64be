"""graclus bench: the native matching (ops.graclus_match: the incidence build,
the batched rounds, the host reads) against a restatement of the same rounds in
torch device ops -- the priority words as int64 tensors, per round three
scatter_reduce amax passes (the key, the pair, the neighbour) for the pointers,
a gather for the mutual check and one host read of the live count -- on the two
workloads of tools/bench_cluster_pool.py, each unweighted and with the
normalized cut of the edge lengths as weights.  The parent of this layer had no
graclus at all, so the composition is the yardstick.

Timed with device events after a warm-up, in windows of at least --window
seconds, the two variants alternating inside every repeat; then the native
incidence build alone, and the native matching at other rounds-per-read values
(--sweep).  One JSON line per case; --out also writes them to a file with the
native source hash.

    python tools/bench_graclus.py [--out profiles/graclus_bench.json]
"""
import argparse
import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from mi355_mp import _lib, ops  # noqa: E402
from torch_geometric.utils import normalized_cut  # noqa: E402

from bench_cluster_pool import WORKLOADS, window_ms  # noqa: E402

_M64 = (1 << 64) - 1


def _i64(v):
    """A Python integer's low 64 bits as the int64 with that bit pattern."""
    v &= _M64
    return v - (1 << 64) if v >> 63 else v


def _lsr(z, k):
    return (z >> k) & ((1 << (64 - k)) - 1)


def _mix64_t(z):
    z = z + _i64(0x9E3779B97F4A7C15)
    z = (z ^ _lsr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _i64(0x94D049BB133111EB)
    return z ^ _lsr(z, 31)


def torch_graclus(ei, weight, n, seed=0):
    """(cluster, rounds, host reads) of the same rounds in torch device ops."""
    dev = ei.device
    u = torch.cat([ei[0], ei[1]])
    v = torch.cat([ei[1], ei[0]])
    keep = u != v
    a, b = torch.minimum(u, v), torch.maximum(u, v)
    h = _lsr(_mix64_t((a << 32 | b) ^ _i64(ops._mix64(seed & _M64))), 32)
    if weight is None:
        wk = torch.zeros_like(h)
    else:
        bits = torch.cat([weight, weight]).view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        wk = torch.where(bits >> 31 != 0, ~bits & 0xFFFFFFFF, bits | 0x80000000)
    key = ((wk << 32) | h) ^ _i64(1 << 63)           # the unsigned order as a signed one
    u, v, key, pair = u[keep], v[keep], key[keep], (a * n + b)[keep]
    lowest = torch.iinfo(torch.int64).min
    cluster = torch.arange(n, device=dev)
    matched = torch.zeros(n, dtype=torch.bool, device=dev)
    live = torch.zeros(n, dtype=torch.bool, device=dev)
    live[u] = True
    rounds = reads = 0
    reads += 1
    n_live = int(live.sum())
    while n_live:
        rounds += 1
        cand = live[u] & ~matched[v]
        cu, cv, ck, cp = u[cand], v[cand], key[cand], pair[cand]
        best_k = torch.full((n,), lowest, dtype=torch.int64, device=dev).scatter_reduce_(0, cu, ck, "amax")
        top = ck == best_k[cu]
        cu, cv, cp = cu[top], cv[top], cp[top]
        best_p = torch.full((n,), -1, dtype=torch.int64, device=dev).scatter_reduce_(0, cu, cp, "amax")
        top = cp == best_p[cu]
        ptr = torch.full((n,), -1, dtype=torch.int64, device=dev).scatter_reduce_(0, cu[top], cv[top], "amax")
        has = ptr >= 0
        mutual = has & (ptr[ptr.clamp(min=0)] == torch.arange(n, device=dev))
        cluster = torch.where(mutual, torch.minimum(cluster, ptr), cluster)
        matched = matched | mutual
        live = has & ~mutual
        n_live = int(live.sum())
        reads += 1
    return cluster, rounds, reads


def cases(dev):
    for name, build in WORKLOADS:
        w = build(dev)
        ei, pos = w["edge_index"], w["pos"]
        n = int(pos.size(0))
        length = (pos[ei[0]] - pos[ei[1]]).norm(dim=1)
        del w
        yield name + "_unweighted", ei, None, n
        yield name + "_normalized_cut", ei, normalized_cut(ei, length, n), n
        torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated case names")
    ap.add_argument("--sweep", default="1,4,8,16,32", help="rounds-per-read values timed besides the default")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    _lib.load()
    only = set(args.only.split(",")) if args.only else None
    sweep = [int(s) for s in args.sweep.split(",") if s]
    records = []
    for name, ei, weight, n in cases(dev):
        if only and name not in only:
            continue
        with torch.no_grad():
            m = ops.graclus_match(ei, weight, n)
            t_cluster, t_rounds, t_reads = torch_graclus(ei, weight, n)
            steps = {"native": lambda: ops.graclus_match(ei, weight, n),
                     "torch_ops": lambda: torch_graclus(ei, weight, n)}
            for s in steps.values():
                for _ in range(3):
                    s()
            torch.cuda.synchronize()
            times = {k: [] for k in steps}
            for _ in range(args.repeats):
                for k, s in steps.items():
                    times[k].append(window_ms(s, args.window))
            build_ms = window_ms(lambda: ops.graclus_incidence(ei, n), args.window / 4)
            by_r = {}
            for r in sweep:
                by_r[str(r)] = {"ms": round(window_ms(lambda: ops.graclus_match(ei, weight, n, rounds_per_read=r),
                                                      args.window / 4), 4),
                                "host_reads": ops.graclus_match(ei, weight, n, rounds_per_read=r).host_reads}
        pairs = int((m.cluster != torch.arange(n, device=dev)).sum())
        rec = {"case": name, "N": n, "E": int(ei.size(1)), "weighted": weight is not None, "pairs": pairs,
               "rounds": m.rounds, "host_reads": m.host_reads, "launches": m.launches,
               "rounds_per_read": ops.GRACLUS_ROUNDS_PER_READ, "torch_rounds": t_rounds, "torch_host_reads": t_reads,
               "same_cluster_as_torch_ops": bool(torch.equal(m.cluster, t_cluster)),
               "native_incidence_build_ms": round(build_ms, 4), "native_ms_by_rounds_per_read": by_r,
               "source_hash": _lib.source_hash()}
        for k, v in times.items():
            v = sorted(v)
            rec[k + "_ms"] = round(v[len(v) // 2], 4)
            rec[k + "_spread_ms"] = round(v[-1] - v[0], 4)
        print(json.dumps(rec), flush=True)
        records.append(rec)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0),
                       "window_s": args.window, "repeats": args.repeats, "records": records}, fh, indent=1)
            fh.write("\n")
    return records


if __name__ == "__main__":
    main()
