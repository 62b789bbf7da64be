"""Point-set bench: the native fps, radius, edge-feature kernel and one whole set
abstraction stage (csrc/mp_point.hip) against the upstream recipes written in
torch device ops, in the same process on the same commit:

  fps     a Python loop of k - 1 steps over the padded batch [B, n, D]: the squared
          distance to the last selection in elementwise ops (the kernels'
          arithmetic, so the two select the same points), minimum, argmax;
  radius  the padded batched distance matrix [B, n_y, n_x], the mask d2 <= r2, its
          cumulative count along x, and the entries with count <= cap;
  edges   the generic path's three native row gathers, the subtraction and the cat;
  stage   fps + radius + PointConv (forward and backward) against recipe fps +
          recipe radius + PointConv through the generic MessagePassing path.

Two shapes: the example's (32 clouds of 1024 points, then of 512: ratios 0.5 / 0.25,
r 0.1 / 0.2, cap 64) and one cloud of 2^16 points (ratio 1/16, r 0.1, cap 32).
Native and recipe must agree (asserted) before anything is timed.  Timed with
device events after a warm-up, in windows of at least --window seconds, native and
recipe alternating inside every repeat; the median and the spread (max - min) of
the repeats are reported.  One JSON line per case; --out also writes them to a
file with the native source hash.

    python tools/bench_point.py [--out profiles/point_bench.json]
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
from torch_geometric.nn import PointConv  # noqa: E402

from bench_cluster_pool import window_ms  # noqa: E402


def d2_to(points, centre):
    """[..., n]: the kernels' squared distance of points [..., n, D] to centre [..., 1, D]."""
    t = points[..., 0] - centre[..., 0]
    acc = t * t
    for d in range(1, points.shape[-1]):
        t = points[..., d] - centre[..., d]
        acc = acc + t * t
    return acc


def torch_fps(pos, B, ratio):
    """idx [B * k] of B equal clouds, every cloud starting at its first point."""
    n = pos.shape[0] // B
    k = min(n, int(torch.ceil(torch.tensor(ratio, dtype=torch.float32) * torch.tensor(n, dtype=torch.float32))))
    p = pos.view(B, n, -1)
    ar = torch.arange(B, device=pos.device)
    m = torch.full((B, n), float("inf"), device=pos.device)
    cur = torch.zeros(B, dtype=torch.int64, device=pos.device)
    out = [cur]
    for _ in range(1, k):
        m = torch.minimum(m, d2_to(p, p[ar, cur].unsqueeze(1)))
        cur = m.argmax(1)
        out.append(cur)
    return (torch.stack(out, 1) + (ar * n).unsqueeze(1)).reshape(-1)


def torch_radius(x, y, r, B, cap):
    """[2, E] of B equal clouds on both sides."""
    n_x, n_y = x.shape[0] // B, y.shape[0] // B
    r2 = torch.tensor(r, dtype=torch.float32) * torch.tensor(r, dtype=torch.float32)
    xs, ys = x.view(B, 1, n_x, -1), y.view(B, n_y, 1, -1)
    mask = d2_to(xs, ys) <= r2.to(x.device)
    keep = mask & (mask.cumsum(-1) <= cap)
    b, j, i = keep.nonzero(as_tuple=True)
    return torch.stack([b * n_y + j, b * n_x + i])


def generic_edge_features(x, pos, centre, src, dst):
    rel = ops.index_select_rows(pos, src) - ops.index_select_rows(centre, dst)
    return rel if x is None else torch.cat([ops.index_select_rows(x, src), rel], dim=1)


class GenericPointConv(PointConv):
    """PointConv through MessagePassing's generic path (an overridden message())."""

    def message(self, x_j, pos_i, pos_j):
        return PointConv.message(self, x_j, pos_i, pos_j)


def mlp(*widths):
    layers = []
    for a, b in zip(widths[:-1], widths[1:]):
        layers += [torch.nn.Linear(a, b), torch.nn.ReLU()]
    return torch.nn.Sequential(*layers[:-1])


def shapes(dev):
    g = torch.Generator().manual_seed(0)
    clouds = torch.rand(32 * 1024, 3, generator=g) * 2 - 1
    big = torch.rand(1 << 16, 3, generator=g) * 2 - 1
    feat = torch.randn(32 * 512, 128, generator=g)
    yield {"name": "example_sa1", "pos": clouds.to(dev), "B": 32, "ratio": 0.5, "r": 0.1, "cap": 64, "x": None,
           "nn": (3, 64, 64, 128)}
    yield {"name": "example_sa2", "pos": clouds[:32 * 512].to(dev), "B": 32, "ratio": 0.25, "r": 0.2, "cap": 64,
           "x": feat.to(dev), "nn": (131, 128, 128, 256)}
    yield {"name": "cloud_2e16", "pos": big.to(dev), "B": 1, "ratio": 1.0 / 16, "r": 0.1, "cap": 32, "x": None,
           "nn": (3, 64, 64, 128)}


def timed(steps, window, repeats, warm=3):
    for s in steps.values():
        for _ in range(warm):
            s()
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(repeats):
        for k, s in steps.items():
            times[k].append(window_ms(s, window))
    out = {}
    for k, v in times.items():
        v = sorted(v)
        out[k + "_ms"] = round(v[len(v) // 2], 4)
        out[k + "_spread_ms"] = round(v[-1] - v[0], 4)
    return out


def verdict(rec):
    """native is not slower than the recipe beyond the spread the repeats showed"""
    slack = max(rec["native_spread_ms"], rec["recipe_spread_ms"])
    rec["recipe_over_native"] = round(rec["recipe_ms"] / rec["native_ms"], 3)
    rec["native_not_slower"] = bool(rec["native_ms"] <= rec["recipe_ms"] + slack)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated shape names")
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

    for sh in shapes(dev):
        if only and sh["name"] not in only:
            continue
        pos, B, ratio, r, cap, x = sh["pos"], sh["B"], sh["ratio"], sh["r"], sh["cap"], sh["x"]
        n = pos.shape[0]
        batch = torch.arange(B, device=dev).repeat_interleave(n // B)
        base = {"shape": sh["name"], "clouds": B, "points": n // B, "ratio": ratio, "r": r, "cap": cap}

        # fps
        with torch.no_grad():
            idx = ops.fps(pos, batch, ratio)
            assert torch.equal(idx, torch_fps(pos, B, ratio)), "fps: native and recipe differ"
            rec = dict(base, piece="fps", K=int(idx.numel()), path=ops.fps_path(n // B))
            rec.update(timed({"native": lambda: ops.fps(pos, batch, ratio), "recipe": lambda: torch_fps(pos, B, ratio)},
                             args.window, args.repeats))
        emit(verdict(rec))

        # radius
        centre, centre_batch = pos[idx], batch[idx]
        with torch.no_grad():
            found = ops.radius_search(pos, centre, r, batch, centre_batch, cap)
            assert torch.equal(found, torch_radius(pos, centre, r, B, cap)), "radius: native and recipe differ"
            per_query = torch.bincount(found[0], minlength=centre.shape[0])
            rec = dict(base, piece="radius", E=int(found.shape[1]), queries=int(centre.shape[0]),
                       queries_at_cap=int((per_query == cap).sum()))
            rec.update(timed({"native": lambda: ops.radius_search(pos, centre, r, batch, centre_batch, cap),
                              "recipe": lambda: torch_radius(pos, centre, r, B, cap)}, args.window, args.repeats))
        emit(verdict(rec))

        # edge features, forward and forward + backward
        src, dst = found[1].contiguous(), found[0].contiguous()
        with torch.no_grad():
            assert torch.equal(ops.point_edge_features(x, pos, centre, src, dst),
                               generic_edge_features(x, pos, centre, src, dst)), "edge features differ"
            rec = dict(base, piece="edge_features_forward", E=int(src.numel()), F=0 if x is None else int(x.shape[1]))
            rec.update(timed({"native": lambda: ops.point_edge_features(x, pos, centre, src, dst),
                              "recipe": lambda: generic_edge_features(x, pos, centre, src, dst)},
                             args.window, args.repeats))
        emit(verdict(rec))
        pg = pos.clone().requires_grad_(True)
        xg = None if x is None else x.clone().requires_grad_(True)

        def both_ways(f):
            def step():
                pg.grad = None
                f(xg, pg, centre, src, dst).sum().backward()
            return step
        rec = dict(base, piece="edge_features_forward_backward", E=int(src.numel()), F=0 if x is None else int(x.shape[1]))
        rec.update(timed({"native": both_ways(ops.point_edge_features), "recipe": both_ways(generic_edge_features)},
                         args.window, args.repeats))
        emit(verdict(rec))

        # one set-abstraction stage, forward and backward
        torch.manual_seed(0)
        local_nn = mlp(*sh["nn"]).to(dev)
        layers = {"native": PointConv(local_nn), "recipe": GenericPointConv(local_nn)}

        def stage(kind):
            layer = layers[kind]

            def step():
                if kind == "native":
                    i = ops.fps(pos, batch, ratio)
                    c, cb = pos[i], batch[i]
                    e = ops.radius_search(pos, c, r, batch, cb, cap).flip(0)
                else:
                    i = torch_fps(pos, B, ratio)
                    c = pos[i]
                    e = torch_radius(pos, c, r, B, cap).flip(0)
                for q in local_nn.parameters():
                    q.grad = None
                if xg is not None:
                    xg.grad = None
                out = layer(xg, (pos, c), e)
                out.sum().backward()
                return out
            return step
        a, b = stage("native")(), stage("recipe")()
        assert a.shape == b.shape and bool(((a - b).abs() <= 1e-5 * b.abs().clamp(min=1.0)).all()), "stage outputs differ"
        rec = dict(base, piece="set_abstraction_forward_backward", E=int(src.numel()))
        rec.update(timed({"native": stage("native"), "recipe": stage("recipe")}, args.window, args.repeats))
        emit(verdict(rec))
        del found, src, dst, pg, xg, layers
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0),
                       "window_s": args.window, "repeats": args.repeats, "records": records}, fh, indent=1)
            fh.write("\n")
    return records


if __name__ == "__main__":
    main()
