"""Input generators shared by the CPU and the GPU fuzz tests of SplineConv,
TopKPooling and cluster pooling (tests/test_fuzz_cases_host.py,
tests/test_gpu_fuzz_pool_layers.py, tests/test_gpu_fuzz_layers.py).

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
