"""Input generators shared by the CPU and the GPU fuzz tests of SplineConv,
TopKPooling, cluster pooling, NNConv and RGCNConv (tests/test_fuzz_cases_host.py,
tests/test_gpu_fuzz_pool_layers.py, tests/test_gpu_fuzz_layers.py,
tests/test_gpu_fuzz_conv_layers.py).

Plain torch on the CPU: every generator takes simple parameters plus a seed and
returns CPU tensors, so a failing example replays from its arguments alone.
"""
import torch

from tests import _cluster_ref, _pool_ref

BATCH_KINDS = ("tiny", "wave", "edge", "random")
SCORE_KINDS = ("distinct", "ties", "five", "equal")
CLUSTER_KINDS = ("voxel", "one", "each", "wide")
CLUSTER_EDGE_KINDS = ("random", "none", "inside", "pairs")
VOXEL_SIZES = (5, 7, 14, 40)
VOXEL_END = 28.0

RELATION_KINDS = ("uniform", "one", "skewed")
NORM_KINDS = (None, "rand", "signed")
FLOWS = ("source_to_target", "target_to_source")

_SIZE_SETS = {"tiny": (0, 1, 2, 3), "wave": (25, 63, 64), "edge": (0, 1, 64, 65, 100, 101, 130)}
_TIES = torch.tensor([-0.5, 0.25, 0.75, 1.5])
_FIVE = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan")])


def graph(N, deg, loops, seed, n_src=None):
    """Random edge list with duplicates; `loops` of its edges made self loops
    (some nodes get several).  n_src: bipartite source count (no loops)."""
    g = torch.Generator().manual_seed(seed)
    E = int(N * deg)
    ns = N if n_src is None else n_src
    ei = torch.stack([torch.randint(ns, (E,), generator=g), torch.randint(N, (E,), generator=g)])
    if E and N > 1 and n_src is None:
        hub = torch.randint(N, (1,), generator=g)
        ei[1, : E // 4] = hub                       # one hub destination
    if loops and E and n_src is None:
        k = max(1, int(E * loops))
        pos = torch.randint(E, (k,), generator=g)
        ei[0, pos] = ei[1, pos]
    return ei, g


def batch_sizes(kind, seed, cap=None):
    """1..12 graph sizes of one kind; empty graphs may lead, trail and repeat, but
    at least one graph has a node (a batch without nodes has no batch vector to
    speak of).  cap: graphs are dropped from the end while the total exceeds it."""
    g = torch.Generator().manual_seed(seed)
    count = int(torch.randint(1, 13, (1,), generator=g))
    if kind == "random":
        sizes = torch.randint(1, 41, (count,), generator=g).tolist()
    else:
        pool = torch.tensor(_SIZE_SETS[kind])
        sizes = pool[torch.randint(len(pool), (count,), generator=g)].tolist()
        if sum(sizes) == 0:
            sizes[int(torch.randint(count, (1,), generator=g))] = int(pool[pool > 0][0])
    while cap is not None and len(sizes) > 1 and sum(sizes) > cap:
        sizes.pop()
    return sizes


def visible(sizes):
    """The sizes a batch vector can carry: trailing empty graphs leave no id behind
    (the number of graphs is batch[-1] + 1)."""
    sizes = list(sizes)
    while sizes and sizes[-1] == 0:
        sizes.pop()
    return sizes


def scores(kind, n, seed):
    """n float32 scores: distinct values, few repeated values, the five special
    values (0.0, -0.0, +inf, -inf, NaN), or one value."""
    g = torch.Generator().manual_seed(seed)
    if kind == "distinct":
        return _pool_ref.distinct_scores(n, g) if n else torch.empty(0)
    if kind == "ties":
        return _TIES[torch.randint(4, (n,), generator=g)]
    if kind == "five":
        return _FIVE[torch.randint(5, (n,), generator=g)]
    if kind == "equal":
        return torch.full((n,), 0.25)
    raise ValueError(kind)


def pseudo(E, D, ks, seed):
    """Random coordinates in [0, 1] with exact 0, 1 and grid points k / ks."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(E, D, generator=g)
    u[0::17] = 0.0
    u[1::17] = 1.0
    for d in range(D):
        k = torch.randint(0, ks[d] + 1, (len(u[2::17]),), generator=g)
        u[2::17, d] = k.float() / ks[d]
    return u


def clusters(kind, n, batch, seed, D=2):
    """(cluster int64 [n], pos float32 [n, D], voxel size or None).  pos lies in
    [0, 28)^D for every kind; for "voxel" the cluster vector is the restatement's
    voxel_grid(pos, batch, size, 0, 28)."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(n, D, generator=g) * (VOXEL_END - 0.01)
    if kind == "voxel":
        size = VOXEL_SIZES[int(torch.randint(len(VOXEL_SIZES), (1,), generator=g))]
        return _cluster_ref.voxel_grid(pos, batch, size, 0, VOXEL_END), pos, size
    if kind == "one":
        return torch.full((n,), 7, dtype=torch.int64), pos, None
    if kind == "each":
        return torch.randperm(n, generator=g) * 3 - 5, pos, None
    if kind == "wide":
        m = max(1, n // 3)
        vals = torch.randint(-(1 << 62), 1 << 62, (m,), generator=g)
        return vals[torch.randint(m, (n,), generator=g)], pos, None
    raise ValueError(kind)


def cluster_edges(kind, n, cluster, seed):
    """edge_index int64 [2, E] over n >= 1 nodes."""
    g = torch.Generator().manual_seed(seed)
    if kind == "none":
        return torch.empty((2, 0), dtype=torch.int64)
    E = 4 * n + 3
    if kind == "random":
        ei = torch.randint(n, (2, E), generator=g)
        ei[1, ::7] = ei[0, ::7]                        # self loops
        ei[:, 1::5] = ei[:, 0:1]                       # duplicates of the first edge
        return ei
    if kind == "inside":
        # the second end is a random member of the first end's cluster
        order = torch.argsort(cluster, stable=True)
        _, inv, cnt = torch.unique(cluster, return_inverse=True, return_counts=True)
        first = torch.cat([cnt.new_zeros(1), cnt.cumsum(0)[:-1]])
        src = torch.randint(n, (E,), generator=g)
        c = inv[src]
        off = (torch.rand(E, generator=g) * cnt[c]).long().clamp(max=cnt[c] - 1)
        return torch.stack([src, order[first[c] + off]])
    if kind == "pairs":
        few = torch.randint(n, (2, 3), generator=g)
        return few[:, torch.randint(3, (E,), generator=g)]
    raise ValueError(kind)


def relations(kind, E, R, seed):
    """edge_type int64 [E] in [0, R): "uniform"; "one": every edge in one relation,
    which is not 0 when R > 1; "skewed": 1 / k frequencies over the relations but
    relation 1, which stays empty, when R > 2 (over both when R = 2)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "uniform":
        return torch.randint(R, (E,), generator=g)
    if kind == "one":
        return torch.full((E,), 0 if R == 1 else 1 + seed % (R - 1), dtype=torch.int64)
    if kind == "skewed":
        used = torch.tensor([r for r in range(R) if r != 1 or R <= 2])
        freq = 1.0 / torch.arange(1, used.numel() + 1, dtype=torch.float64)
        if E == 0:
            return torch.empty(0, dtype=torch.int64)
        return used[torch.multinomial(freq / freq.sum(), E, replacement=True, generator=g)]
    raise ValueError(kind)


def edge_norm(kind, E, seed):
    """None, or float32 [E]: "rand" in [0.5, 1.5); "signed": values in (-1, 1) with
    exact zeros, exact ones and negatives mixed in (every third edge 0, every
    third edge + 1 a 1)."""
    if kind is None:
        return None
    g = torch.Generator().manual_seed(seed)
    if kind == "rand":
        return torch.rand(E, generator=g) + 0.5
    if kind == "signed":
        w = torch.rand(E, generator=g) * 2 - 1
        w[0::3] = 0.0
        w[1::3] = 1.0
        w[2::6] = -w[2::6].abs() - 0.25
        return w
    raise ValueError(kind)


def edge_attr(E, D, seed):
    """float32 [E, D] in [0, 1] with exact all-0 rows (every 7th) and all-1 rows (every 7th + 1)."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(E, D, generator=g)
    u[0::7] = 0.0
    u[1::7] = 1.0
    return u


def _nn(N, deg, loops, c_in, c_out, H, D, aggr, flow, root, bias, head_bias, form, nn, seed):
    return dict(N=N, deg=deg, loops=loops, c_in=c_in, c_out=c_out, H=H, D=D, aggr=aggr, flow=flow, root=root,
                bias=bias, head_bias=head_bias, form=form, nn=nn, seed=seed)


# The pinned examples of test_fuzz_nnconv_layer: N = 1 without edges and with self loops only; E = 0 (root and
# bias alone); every edge a loop; mean with isolated nodes (deg 0.3); a bare Linear whose edge_attr gradient is
# the edge-gradient kernel's output at (Cin, H) = (33, 40) (64 lanes, one partial tile), (70, 40) (32 lanes, a
# partial tile after a full one) and (32, 25) (the grouped kernel's widest group); gather without a head bias
NNCONV_PINNED = (
    _nn(1, 0.0, 0.0, 5, 3, 4, 3, "add", FLOWS[0], True, True, True, None, "mlp", 1),
    _nn(1, 3.0, 1.0, 2, 8, 4, 1, "mean", FLOWS[0], True, True, True, "bins", "mlp", 2),
    _nn(5, 0.0, 0.0, 5, 3, 4, 3, "add", FLOWS[1], True, True, True, "gather", "mlp", 3),
    _nn(5, 0.0, 0.0, 16, 8, 4, 3, "mean", FLOWS[0], True, True, True, "bins", "linear", 4),
    _nn(40, 4.0, 1.0, 16, 3, 25, 3, "add", FLOWS[0], True, False, True, "gather", "mlp", 5),
    _nn(60, 0.3, 0.0, 5, 33, 4, 1, "mean", FLOWS[1], False, True, True, "bins", "mlp", 6),
    _nn(50, 4.0, 0.2, 33, 3, 40, 1, "add", FLOWS[0], True, True, True, "bins", "linear", 7),
    _nn(50, 4.0, 0.2, 70, 1, 40, 1, "mean", FLOWS[1], True, True, True, "gather", "linear", 8),
    _nn(50, 4.0, 0.2, 32, 8, 25, 1, "add", FLOWS[0], False, False, True, None, "linear", 9),
    _nn(70, 6.0, 0.2, 70, 3, 4, 3, "mean", FLOWS[0], True, True, False, "gather", "mlp", 10),
)


def _rg(N, deg, loops, c_in, c_out, R, B, rkind, nkind, mode, flow, root, bias, seed):
    return dict(N=N, deg=deg, loops=loops, c_in=c_in, c_out=c_out, R=R, B=B, rkind=rkind, nkind=nkind, mode=mode,
                flow=flow, root=root, bias=bias, seed=seed)


# The pinned examples of test_fuzz_rgcnconv_layer: N = 1 without edges, featured and featureless; E = 0; one
# relation; B = 65 (a second tile of the att gradient) with three columns; every edge in one relation, which
# then spans more than two chunks of the att gradient; every edge a loop; a signed norm with zeros and ones
RGCN_PINNED = (
    _rg(1, 0.0, 0.0, 3, 4, 2, 2, "uniform", None, "chosen", FLOWS[0], True, True, 1),
    _rg(1, 0.0, 0.0, 3, 4, 7, 5, "uniform", "rand", "featureless", FLOWS[0], True, True, 2),
    _rg(5, 0.0, 0.0, 16, 4, 7, 5, "skewed", "rand", "bins", FLOWS[1], True, True, 3),
    _rg(5, 0.0, 0.0, 16, 4, 7, 5, "skewed", None, "featureless", FLOWS[0], True, True, 4),
    _rg(40, 4.0, 0.2, 16, 33, 1, 5, "uniform", "rand", "gather", FLOWS[0], True, False, 5),
    _rg(60, 4.0, 0.2, 3, 4, 7, 65, "skewed", "rand", "bins", FLOWS[1], False, True, 6),
    _rg(80, 8.0, 0.2, 3, 4, 7, 17, "one", "rand", "chosen", FLOWS[0], True, True, 7),
    _rg(80, 8.0, 0.0, 1, 70, 30, 2, "one", None, "featureless", FLOWS[1], True, True, 8),
    _rg(40, 4.0, 1.0, 32, 4, 2, 5, "uniform", None, "gather", FLOWS[0], True, True, 9),
    _rg(50, 4.0, 0.2, 33, 1, 30, 17, "skewed", "signed", "bins", FLOWS[0], True, True, 10),
    _rg(50, 4.0, 0.2, 3, 70, 7, 2, "uniform", "signed", "featureless", FLOWS[1], False, False, 11),
)


def conv_graph(N, deg, loops, seed):
    """graph(N, deg, loops, seed); loops = 1.0: every edge a self loop (graph()
    draws the loop positions with replacement and leaves some edges as they are)."""
    ei, g = graph(N, deg, loops, seed)
    if loops == 1.0:
        ei[0] = ei[1]
    return ei, g


def nnconv_inputs(p):
    """(edge_index, x [N, c_in], edge_attr [E, D]) of one test_fuzz_nnconv_layer
    draw; a bare Linear ("linear") reads edge_attr as h, so D = H there."""
    ei, g = conv_graph(p["N"], p["deg"], p["loops"], p["seed"])
    D = p["H"] if p["nn"] == "linear" else p["D"]
    x = torch.randn(p["N"], p["c_in"], generator=g)
    return ei, x, edge_attr(ei.shape[1], D, p["seed"])


def rgcn_inputs(p):
    """(edge_index, x [N, c_in] or None, edge_type, edge_norm or None) of one
    test_fuzz_rgcnconv_layer draw; the featureless mode has x = None (and the
    layer in_channels = N)."""
    ei, g = conv_graph(p["N"], p["deg"], p["loops"], p["seed"])
    E = ei.shape[1]
    x = None if p["mode"] == "featureless" else torch.randn(p["N"], p["c_in"], generator=g)
    return ei, x, relations(p["rkind"], E, p["R"], p["seed"]), edge_norm(p["nkind"], E, p["seed"])
