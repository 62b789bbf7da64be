"""Sparse product bench: (A + I)^2 by the native product (csrc/mp_spgemm.hip, through
mi355_mp.ops.spgemm with the row CSR builds and the one host read it makes) against
torch.sparse.mm on coalesced COO tensors on the same GPU -- recorded as unavailable
where the ROCm build refuses a sparse x sparse product.

Graphs: the Cora-shaped graph of examples/graph_unet.py (2708 nodes) and a power-law
graph of 100 k nodes and 1 M edges (mi355_mp.graphgen).

Per variant: one whole product, timed with device events after a warm-up, in windows
of at least --window seconds, the variants alternating inside every repeat (median
and max - min over the repeats), and the peak device memory of one product above what
was allocated before it.  The native product's rows per bin and nnz(C) are recorded.
One JSON line per graph; --out also writes them to a file with the native source hash.

    python tools/bench_spgemm.py [--out profiles/spgemm_bench.json]
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
from torch_geometric.utils import add_self_loops  # noqa: E402

WORKLOADS = [("spgemm_cora", "cora", 2708), ("spgemm_100k_1m", "large", 100_000)]


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
    for name, which, n in WORKLOADS:
        if only and name not in only:
            continue
        ei = cora_like()["edge_index"].to(dev) if which == "cora" else \
            powerlaw_edge_index(n, 1_000_000, seed=3, device=dev)
        ei = torch.unique(ei[0] * n + ei[1])                        # coalesced, as torch.sparse.mm wants it
        ei = torch.stack([ei // n, ei % n])
        ei, w = add_self_loops(ei, torch.ones(ei.shape[1], device=dev), num_nodes=n)
        idx, val, st = ops.spgemm(ei, w, ei, w, n, n, n, want_stats=True)
        rec = {"workload": name, "N": n, "nnz_A": int(ei.shape[1]), "nnz_C": st.nnz,
               "rows_per_bin": {"wave": st.rows_wave, "workgroup": st.rows_workgroup, "window": st.rows_window},
               "launches": st.launches, "bin_caps": {k: ops.spgemm_bin_cap(k) for k in ("wave", "workgroup", "window")},
               "source_hash": _lib.source_hash()}
        steps = {"native": lambda: ops.spgemm(ei, w, ei, w, n, n, n)}
        S = torch.sparse_coo_tensor(ei, w, (n, n)).coalesce()
        try:
            C = torch.sparse.mm(S, S).coalesce()
            same = C._nnz() == st.nnz and bool((C.indices() == idx).all()) and bool((C.values() == val).all())
            rec["torch_sparse_mm"] = "available"
            rec["equal_to_torch_sparse_mm"] = same
            steps["torch_sparse_mm"] = lambda: torch.sparse.mm(S, S)
        except (RuntimeError, NotImplementedError) as e:
            rec["torch_sparse_mm"] = "unavailable: %s" % str(e).splitlines()[0][:200]
        for step in steps.values():
            for _ in range(3):
                step()
        torch.cuda.synchronize()
        times = {k: [] for k in steps}
        for _ in range(args.repeats):
            for k, step in steps.items():
                times[k].append(window_ms(step, args.window))
        for k, v in times.items():
            v = sorted(v)
            rec["%s_ms" % k] = round(v[len(v) // 2], 4)
            rec["%s_spread_ms" % k] = round(v[-1] - v[0], 4)
        for k, step in steps.items():
            rec["%s_peak_bytes" % k] = peak_bytes(step)
        print(json.dumps(rec), flush=True)
        records.append(rec)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0),
                       "window_s": args.window, "repeats": args.repeats, "records": records}, fh, indent=1)
            fh.write("\n")
    return records


if __name__ == "__main__":
    main()
