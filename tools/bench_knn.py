"""Nearest-neighbour bench: the native knn, knn_graph, knn_interpolate and one
feature-propagation stage (csrc/mp_knn.hip) against upstream's recipe written in
torch device ops, in the same process on the same commit:

  knn          the batched distance matrix of equal clouds, torch.cdist over
               [B, n_y, D] x [B, n_x, D], then topk(k, largest=False) along x (one
               cloud of 2^16: in blocks of 8192 queries, so the matrix stays at 2 GiB);
  knn_graph    the same with k + 1 and the point itself dropped;
  interpolate  upstream's knn_interpolate over that knn: gather the k rows, the
               squared distances from the gathered positions, w = 1 / clamp(d2, 1e-16),
               index_add_ of w * x and of w by the query, a division; the backward is
               autograd's;
  stage        interpolate, cat with the skip features, a two-layer MLP, forward and
               backward.

Shapes: the example's (32 clouds of 1024 points, D = 3; the interpolation goes from
every fourth point, 256 a cloud, to all 1024, C = 128), one cloud of 2^16, and
32 x 1024 rows of width 64 for knn_graph at k = 20 (DGCNN's feature-space graph: the
general-width path, which has no bar -- it is recorded, and it is not measured
against a GEMM-based search other than what cdist does inside).

cdist rounds differently from the engine's left-to-right distance, so the two
selections may differ where distances are nearly equal: the share of equal pairs is
recorded and must be above 99.9 %, and the interpolations must agree to 1e-4.
Timed with device events after a warm-up, in windows of at least --window seconds,
native and recipe alternating inside every repeat; the median and the spread
(max - min) of the repeats are reported.  One JSON line per case; --out also writes
them to a file with the native source hash.

    python tools/bench_knn.py [--out profiles/knn_bench.json]
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
from torch_geometric.nn import knn, knn_graph, knn_interpolate  # noqa: E402

from bench_point import mlp, timed, verdict  # noqa: E402

QUERY_BLOCK = 8192


def torch_knn(x, y, k, B):
    """[2, n_y * k] of B equal clouds on both sides: cdist, then topk."""
    n_x, n_y = x.shape[0] // B, y.shape[0] // B
    xs, ys = x.view(B, n_x, -1), y.view(B, n_y, -1)
    cols = []
    for q0 in range(0, n_y, QUERY_BLOCK):
        d = torch.cdist(ys[:, q0:q0 + QUERY_BLOCK], xs)
        cols.append(d.topk(k, dim=-1, largest=False).indices)
    col = torch.cat(cols, dim=1) + (torch.arange(B, device=x.device) * n_x).view(B, 1, 1)
    row = torch.arange(B * n_y, device=x.device).repeat_interleave(k)
    return torch.stack([row, col.reshape(-1)])


def torch_knn_graph(x, k, B):
    row, col = torch_knn(x, x, k + 1, B)
    keep = row != col
    return torch.stack([col[keep], row[keep]])


def torch_interpolate(x, pos_x, pos_y, k, B):
    with torch.no_grad():
        y_idx, x_idx = torch_knn(pos_x, pos_y, k, B)
        diff = pos_x[x_idx] - pos_y[y_idx]
        w = 1.0 / (diff * diff).sum(dim=-1, keepdim=True).clamp(min=1e-16)
    num = torch.zeros(pos_y.shape[0], x.shape[1], device=x.device).index_add_(0, y_idx, x[x_idx] * w)
    den = torch.zeros(pos_y.shape[0], 1, device=x.device).index_add_(0, y_idx, w)
    return num / den


def same_pairs(a, b):
    """the share of (y, x) pairs of a that b holds too (both hold k per query)"""
    n = int(max(a[1].max(), b[1].max())) + 1
    ka, kb = (a[0] * n + a[1]).sort().values, (b[0] * n + b[1]).sort().values
    return float(torch.isin(ka, kb).float().mean())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated pieces: knn, knn_graph, interpolate, stage")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    _lib.load()
    only = set(args.only.split(",")) if args.only else None
    records = []

    def emit(rec, bar):
        rec["source_hash"] = _lib.source_hash()
        rec["bar"] = bar
        print(json.dumps(rec), flush=True)
        records.append(rec)

    g = torch.Generator().manual_seed(0)
    clouds = (torch.rand(32 * 1024, 3, generator=g) * 2 - 1).to(dev)
    big = (torch.rand(1 << 16, 3, generator=g) * 2 - 1).to(dev)
    wide = torch.randn(32 * 1024, 64, generator=g).to(dev)
    feat = torch.randn(32 * 256, 128, generator=g).to(dev)
    skip = torch.randn(32 * 1024, 64, generator=g).to(dev)
    batch = torch.arange(32, device=dev).repeat_interleave(1024)

    # knn
    if not only or "knn" in only:
        for name, pos, B, b in (("example_32x1024", clouds, 32, batch), ("cloud_2e16", big, 1, None)):
            for k in (3, 16):
                with torch.no_grad():
                    found, want = knn(pos, pos, k, b, b), torch_knn(pos, pos, k, B)
                    share = same_pairs(found, want)
                    assert found.shape == want.shape and share > 0.999, "knn: native and recipe differ (%g)" % share
                    rec = {"shape": name, "piece": "knn", "clouds": B, "points": pos.shape[0] // B, "D": 3, "k": k,
                           "E": int(found.shape[1]), "same_pairs": round(share, 6), "path": ops.knn_path(3)}
                    rec.update(timed({"native": lambda: knn(pos, pos, k, b, b), "recipe": lambda: torch_knn(pos, pos, k, B)},
                                     args.window, args.repeats))
                emit(verdict(rec), name == "example_32x1024")

    # knn_graph in feature space: the general-width path, recorded without a bar
    if not only or "knn_graph" in only:
        with torch.no_grad():
            found, want = knn_graph(wide, 20, batch), torch_knn_graph(wide, 20, 32)
            share = same_pairs(found.flip(0), want.flip(0))
            assert share > 0.999, "knn_graph: native and recipe differ (%g)" % share
            rec = {"shape": "features_32x1024", "piece": "knn_graph", "clouds": 32, "points": 1024, "D": 64, "k": 20,
                   "E": int(found.shape[1]), "same_pairs": round(share, 6), "path": ops.knn_path(64)}
            rec.update(timed({"native": lambda: knn_graph(wide, 20, batch), "recipe": lambda: torch_knn_graph(wide, 20, 32)},
                             args.window, args.repeats))
        emit(verdict(rec), False)

    # knn_interpolate: from every fourth point of a cloud to all of them, C = 128
    coarse = clouds.view(32, 1024, 3)[:, ::4].reshape(-1, 3).contiguous()
    coarse_batch = torch.arange(32, device=dev).repeat_interleave(256)
    base = {"shape": "example_32x256_to_32x1024", "clouds": 32, "points_x": 256, "points_y": 1024, "D": 3, "k": 3, "C": 128}
    if not only or "interpolate" in only:
        with torch.no_grad():
            a = knn_interpolate(feat, coarse, clouds, coarse_batch, batch, k=3)
            b = torch_interpolate(feat, coarse, clouds, 3, 32)
            err = float((a - b).abs().max())
            assert err < 1e-4, "knn_interpolate: native and recipe differ by %g" % err
            rec = dict(base, piece="interpolate_forward", max_abs_difference=err)
            rec.update(timed({"native": lambda: knn_interpolate(feat, coarse, clouds, coarse_batch, batch, k=3),
                              "recipe": lambda: torch_interpolate(feat, coarse, clouds, 3, 32)}, args.window, args.repeats))
        emit(verdict(rec), True)
        fg = feat.clone().requires_grad_(True)

        def both_ways(f):
            def step():
                fg.grad = None
                f(fg).sum().backward()
            return step
        rec = dict(base, piece="interpolate_forward_backward")
        rec.update(timed({"native": both_ways(lambda t: knn_interpolate(t, coarse, clouds, coarse_batch, batch, k=3)),
                          "recipe": both_ways(lambda t: torch_interpolate(t, coarse, clouds, 3, 32))},
                         args.window, args.repeats))
        emit(verdict(rec), True)

    # one feature-propagation stage, forward and backward
    if not only or "stage" in only:
        torch.manual_seed(0)
        net = mlp(128 + 64, 128, 128).to(dev)
        fg = feat.clone().requires_grad_(True)

        def stage(kind):
            def step():
                fg.grad = None
                for q in net.parameters():
                    q.grad = None
                if kind == "native":
                    up = knn_interpolate(fg, coarse, clouds, coarse_batch, batch, k=3)
                else:
                    up = torch_interpolate(fg, coarse, clouds, 3, 32)
                out = net(torch.cat([up, skip], dim=1)).relu()
                out.sum().backward()
                return out
            return step
        a, b = stage("native")(), stage("recipe")()
        assert bool(((a - b).abs() <= 1e-4 * b.abs().clamp(min=1.0)).all()), "stage outputs differ"
        rec = dict(base, piece="feature_propagation_forward_backward", skip=64, nn=[192, 128, 128])
        rec.update(timed({"native": stage("native"), "recipe": stage("recipe")}, args.window, args.repeats))
        emit(verdict(rec), True)

    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0),
                       "window_s": args.window, "repeats": args.repeats, "records": records}, fh, indent=1)
            fh.write("\n")
    return records


if __name__ == "__main__":
    main()
