"""Link-prediction bench: GAE's reconstruction loss (forward + backward) and the
negative sampler on the native kernels (csrc/mp_link.hip) against upstream's recipe,
in the same process on the same commit:

  loss      upstream's composition in torch device ops: z.index_select on both ends
            (two [E, C] arrays a side), multiply, sum, sigmoid, log, mean, and
            autograd's backward through the two index_selects (atomic scatters);
            the negatives are the same tensor for both, drawn beforehand;
  sampler   upstream's negative_sampling: the keys copied to the host, Python's
            random.sample, np.isin in a retry loop, the result copied back -- on the
            host clock, since that is where it runs.

Shapes: the example's (a Cora-shaped graph, C = 16) and one whose z (2^20 x 64 fp32,
256 MiB) does not fit the 4 MiB L2 of an XCD, with 2^22 edges a side.  Per case: the
times, the peak device memory of one step over what was allocated before it, and
the host synchronisations of one step (torch's sync debug mode set to warn, the
warnings counted).  Then the lane sweep: mp_edge_score_f32 at every forced lanes
per edge for C = 16, 64 and 128 on the large graph, with the library's own pick.

Timed with device events after a warm-up, in windows of at least --window seconds,
native and recipe alternating inside every repeat; the median and the spread (max -
min) of the repeats are reported.  One JSON line per case; --out also writes them
to a file with the native source hash.

    python tools/bench_link.py [--out profiles/link_bench.json]
"""
import argparse
import json
import os
import random
import sys
import time
import warnings

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "pytorch_geometric-1_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mi355_mp import _lib, ops  # noqa: E402
from mi355_mp.graphgen import cora_like  # noqa: E402

from bench_dna import peak_bytes, window_ms  # noqa: E402
from bench_point import timed, verdict  # noqa: E402

EPS = 1e-15


def recipe_loss(z, pos, neg):
    def side(ei, positive):
        p = torch.sigmoid((z.index_select(0, ei[0]) * z.index_select(0, ei[1])).sum(dim=1))
        return -torch.log((p if positive else 1 - p) + EPS).mean()
    return side(pos, True) + side(neg, False)


def recipe_sampler(edge_index, n):
    """PyG 1.4.x utils.negative_sampling, as written upstream."""
    num = min(edge_index.size(1), n * n - edge_index.size(1))
    idx = (edge_index[0] * n + edge_index[1]).to("cpu")
    rng = range(n * n)
    perm = torch.tensor(random.sample(rng, num))
    mask = torch.from_numpy(np.isin(perm, idx)).to(torch.bool)
    rest = mask.nonzero().view(-1)
    while rest.numel() > 0:
        tmp = torch.tensor(random.sample(rng, rest.size(0)))
        mask = torch.from_numpy(np.isin(tmp, idx)).to(torch.bool)
        perm[rest] = tmp
        rest = rest[mask.nonzero().view(-1)]
    row, col = torch.div(perm, n, rounding_mode="floor"), perm % n
    return torch.stack([row, col], dim=0).long().to(edge_index.device)


def host_syncs(step):
    """Host synchronisations of one call of step (torch's sync debug mode)."""
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            step()
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    return sum("called a synchronizing" in str(w.message) for w in seen)


def host_ms(step, calls):
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated pieces: loss, sampler, lanes")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    _lib.load()
    only = set(args.only.split(",")) if args.only else None
    records = []

    def emit(rec):
        rec["source_hash"] = _lib.source_hash()
        print(json.dumps(rec), flush=True)
        records.append(rec)

    g = torch.Generator().manual_seed(0)
    cora = cora_like()["edge_index"]
    big_n, big_e = 1 << 20, 1 << 22
    shapes = (("example_cora", 2708, 16, cora.to(dev), 3),
              ("z_256MiB", big_n, 64, torch.randint(0, big_n, (2, big_e), generator=g).to(dev), 1))

    for name, n, C, pos, sampler_calls in shapes:
        E = int(pos.shape[1])
        z0 = (torch.randn(n, C, generator=g) * 0.3).to(dev)
        base = {"shape": name, "N": n, "C": C, "E_pos": E, "z_bytes": n * C * 4}

        if not only or "loss" in only:
            neg = ops.negative_sample(pos, n, loops=True, seed=1)
            zg = z0.clone().requires_grad_(True)

            def step(f):
                def run():
                    zg.grad = None
                    f(zg).backward()
                    return zg.grad
                return run
            native, recipe = step(lambda t: ops.link_loss(t, pos, neg, neg_trusted=True)), step(lambda t: recipe_loss(t, pos, neg))
            with torch.no_grad():
                la, lb = float(ops.link_loss(z0, pos, neg, neg_trusted=True)), float(recipe_loss(z0, pos, neg))
            ga, gb = native().clone(), recipe().clone()
            rec = dict(base, piece="recon_loss_forward_backward", E_neg=int(neg.shape[1]), loss_native=la, loss_recipe=lb,
                       max_abs_grad_difference=float((ga - gb).abs().max()), max_abs_grad=float(gb.abs().max()))
            assert abs(la - lb) <= 1e-4 * max(1.0, abs(lb)), "loss: native and recipe differ (%g, %g)" % (la, lb)
            rec.update(timed({"native": native, "recipe": recipe}, args.window, args.repeats))
            rec["native_peak_bytes"], rec["recipe_peak_bytes"] = peak_bytes(native), peak_bytes(recipe)
            rec["native_host_syncs"], rec["recipe_host_syncs"] = host_syncs(native), host_syncs(recipe)

            # the whole training-step piece: sampling included, as GAE.recon_loss runs it
            def native_step():
                zg.grad = None
                ops.link_loss(zg, pos, ops.negative_sample(pos, n, loops=True), neg_trusted=True).backward()
            native_step()
            rec["native_with_sampling_ms"] = round(window_ms(native_step, args.window), 4)
            rec["native_with_sampling_host_syncs"] = host_syncs(native_step)
            emit(verdict(rec))
            del neg, zg, ga, gb

        if not only or "sampler" in only:
            ops.negative_sample(pos, n)                              # builds the cached key table
            nat = timed({"native": lambda: ops.negative_sample(pos, n)}, args.window, args.repeats)
            t0 = time.perf_counter()
            ops.forget_index(pos)
            ops.negative_sample(pos, n)
            torch.cuda.synchronize()
            first_ms = (time.perf_counter() - t0) * 1e3
            host = host_ms(lambda: recipe_sampler(pos, n), sampler_calls)
            rec = dict(base, piece="negative_sampling", n_samples=min(E, n * n - E), native_ms=nat["native_ms"],
                       native_spread_ms=nat["native_spread_ms"], native_first_call_ms=round(first_ms, 4),
                       recipe_ms=round(host[len(host) // 2], 4), recipe_spread_ms=round(host[-1] - host[0], 4),
                       recipe_calls=sampler_calls, recipe_clock="host",
                       native_host_syncs=host_syncs(lambda: ops.negative_sample(pos, n)),
                       recipe_host_syncs=host_syncs(lambda: recipe_sampler(pos, n)))
            emit(verdict(rec))

    if not only or "lanes" in only:
        row, col = shapes[1][3][0].contiguous(), shapes[1][3][1].contiguous()
        for C in (16, 64, 128):
            z = torch.randn(big_n, C, generator=g).to(dev)
            want = ops.edge_score_forward(z, row, col)
            steps = {}
            for lanes in (1, 2, 4, 8, 16, 32, 64):
                if lanes * 4 > 2 * C:
                    continue
                got = ops.edge_score_forward(z, row, col, lanes=lanes)
                assert bool(((got - want).abs() <= 1e-4 * want.abs().clamp(min=1.0)).all()), (C, lanes)
                steps["lanes_%d" % lanes] = (lambda L: lambda: ops.edge_score_forward(z, row, col, lanes=L))(lanes)
            rec = {"piece": "edge_score_lane_sweep", "N": big_n, "C": C, "E": big_e, "z_bytes": big_n * C * 4,
                   "library_pick": ops.link_lanes(C)}
            rec.update(timed(steps, args.window, args.repeats))
            best = min((k for k in rec if k.startswith("lanes_") and k.endswith("_ms") and "spread" not in k),
                       key=lambda k: rec[k])
            rec["fastest"] = int(best.split("_")[1])
            rec["pick_over_fastest"] = round(rec["lanes_%d_ms" % rec["library_pick"]] / rec[best], 3)
            rec["min_bytes"] = big_e * (2 * C * 4 + 16 + 4)
            rec["pick_GBps"] = round(rec["min_bytes"] / rec["lanes_%d_ms" % rec["library_pick"]] / 1e6, 1)
            emit(rec)
            del z, want

    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0),
                       "window_s": args.window, "repeats": args.repeats, "records": records}, fh, indent=1)
            fh.write("\n")
    return records


if __name__ == "__main__":
    main()
