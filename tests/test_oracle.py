"""CPU tests of the oracle: hand-derived known-answer tests (KATs) of the
torch_scatter 2.0.4 / PyG 1.4.3 semantics, agreement of the oracle's two
independent forms (torch ops vs serial C loop), and the golden fixtures.

Parity is UNPINNED by the reference (no tests / fixtures exist for this path
in /root/reference, and torch_scatter / torch_geometric are not installable
here): the KATs below are the pin, each value derived by hand from the
published semantics quoted in oracle/scatter_ref.py and oracle/pyg_ref.py.
"""
import math
import os

import numpy as np
import pytest
import torch

from oracle import scatter_ref as S
from oracle import pyg_ref as P

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

SRC = torch.tensor([[1., -2.], [3., 5.], [-1., 0.], [3., 7.], [2., -3.]])
IDX = torch.tensor([0, 2, 0, 2, 3])


def test_kat_sum_mean():
    want_sum = torch.tensor([[0., -2.], [0., 0.], [6., 12.], [2., -3.], [0., 0.]])
    want_mean = torch.tensor([[0., -1.], [0., 0.], [3., 6.], [2., -3.], [0., 0.]])
    assert torch.equal(S.scatter_sum(SRC, IDX, 5), want_sum)
    assert torch.equal(S.scatter_loop(SRC, IDX, 5, "sum")[0], want_sum)
    assert torch.equal(S.scatter_mean(SRC, IDX, 5), want_mean)
    assert torch.equal(S.scatter_loop(SRC, IDX, 5, "mean")[0], want_mean)


def test_kat_max_min_first_index_ties_and_empty_rows():
    out, arg = S.scatter_max(SRC, IDX, 5)
    assert torch.equal(out, torch.tensor([[1., 0.], [0., 0.], [3., 7.], [2., -3.], [0., 0.]]))
    # row 2 feature 0: 3 (edge 1) ties 3 (edge 3) -> first edge wins; empty -> E = 5
    assert torch.equal(arg, torch.tensor([[0, 2], [5, 5], [1, 3], [4, 4], [5, 5]]))
    out, arg = S.scatter_min(SRC, IDX, 5)
    assert torch.equal(out, torch.tensor([[-1., -2.], [0., 0.], [3., 5.], [2., -3.], [0., 0.]]))
    assert torch.equal(arg, torch.tensor([[2, 0], [5, 5], [1, 1], [4, 4], [5, 5]]))


def test_kat_max_special_values():
    src = torch.tensor([[float("-inf")], [-20000.], [-5.], [float("nan")]])
    out, arg = S.scatter_max(src, torch.tensor([0, 1, 1, 2]), 4)
    # -inf and nan never beat lowest(): the row stays at init -> 0, arg = E
    assert torch.equal(out, torch.tensor([[0.], [-5.], [0.], [0.]]))
    assert torch.equal(arg, torch.tensor([[4], [2], [4], [4]]))
    # PyG scatter_ masks max < -10000 to 0
    src = torch.tensor([[-20000.], [-30000.]])
    assert S.scatter_max(src, torch.tensor([0, 0]), 1)[0].item() == -20000.
    assert P.scatter_("max", src, torch.tensor([0, 0]), 1).item() == 0.
    assert P.scatter_("min", torch.tensor([[20000.]]), torch.tensor([0]), 1).item() == 0.


def test_kat_out_given():
    out0 = torch.tensor([[10., 10.], [-1., -1.]])
    src = torch.tensor([[1., 2.], [3., 4.]])
    idx = torch.tensor([0, 0])
    s, _ = S.scatter_loop(src, idx, 2, "sum", out=out0)
    assert torch.equal(s, torch.tensor([[14., 16.], [-1., -1.]]))
    m, a = S.scatter_loop(src, idx, 2, "max", out=out0)
    assert torch.equal(m, out0)  # no element beats the given values; no lowest->0 masking
    assert torch.equal(a, torch.tensor([[2, 2], [2, 2]]))


def test_kat_add_remaining_self_loops_and_gcn_norm():
    ei = torch.tensor([[0, 1, 1, 2], [1, 1, 2, 0]])
    w = torch.tensor([1., 2., 3., 4.])
    ei2, w2 = P.add_remaining_self_loops(ei, w, 1, 3)
    assert ei2.tolist() == [[0, 1, 2, 0, 1, 2], [1, 2, 0, 0, 1, 2]]
    assert w2.tolist() == [1., 3., 4., 1., 2., 1.]
    _, norm = P.gcn_norm(ei, 3, w)
    # deg over edge_index[0]: [2, 5, 5]
    want = [1 / math.sqrt(2) / math.sqrt(5), 3 / 5, 4 / math.sqrt(5) / math.sqrt(2), 1 / 2, 2 / 5, 1 / 5]
    assert np.allclose(norm.numpy(), want, rtol=1e-6, atol=0)
    # improved=True: a node WITH a pre-existing loop keeps its weight, others get 2
    ei3, w3 = P.add_remaining_self_loops(ei, torch.ones(4), 2, 3)
    assert w3.tolist() == [1., 1., 1., 2., 1., 2.]


def test_kat_gcn_norm_isolated_node_inf_to_zero():
    # node 0's only edge is a zero-weight self loop, kept as its loop weight:
    # deg(0) = 0 -> deg^-1/2 = inf -> 0, so its norm is 0 (not nan)
    ei2, norm = P.gcn_norm(torch.tensor([[0], [0]]), 2, torch.tensor([0.]))
    assert ei2.tolist() == [[0, 1], [0, 1]]
    assert norm.tolist() == [0.0, 1.0]
    _, n2 = P.gcn_norm(torch.tensor([[0, 1], [1, 0]]), 2, torch.tensor([1., 1.]))
    assert torch.allclose(n2, torch.tensor([0.5, 0.5, 0.5, 0.5]))


def test_kat_remove_add_self_loops_order():
    ei = torch.tensor([[0, 1, 2, 2], [0, 0, 2, 1]])
    e1, _ = P.remove_self_loops(ei)
    assert e1.tolist() == [[1, 2], [0, 1]]
    e2, _ = P.add_self_loops(e1, num_nodes=3)
    assert e2.tolist() == [[1, 2, 0, 1, 2], [0, 1, 0, 1, 2]]


def test_kat_softmax():
    src = torch.tensor([1., 2., 3., 0.5])
    idx = torch.tensor([0, 0, 1, 0])
    out = P.softmax(src, idx, 3)
    z = math.exp(-1) + 1 + math.exp(-1.5)
    want = [math.exp(-1) / z, 1 / z, 1.0, math.exp(-1.5) / z]
    assert np.allclose(out.numpy(), want, rtol=1e-6)


def test_torch_and_loop_forms_agree_on_random_graph():
    g = torch.Generator().manual_seed(5)
    E, N, F = 3000, 300, 17
    src = torch.randn(E, F, generator=g)
    idx = torch.randint(N, (E,), generator=g)
    assert torch.equal(S.scatter_sum(src, idx, N), S.scatter_loop(src, idx, N, "sum")[0])
    assert torch.equal(S.scatter_mean(src, idx, N), S.scatter_loop(src, idx, N, "mean")[0])
    # torch's amax reduction + first-index argmin over ties == the serial loop
    out, arg = S.scatter_max(src, idx, N)
    ref = torch.full((N, F), float("-inf")).scatter_reduce(0, idx.view(-1, 1).expand(E, F), src, "amax")
    ref[torch.isinf(ref)] = 0
    assert torch.equal(out, ref)
    e = torch.arange(E).view(-1, 1).expand(E, F)
    hit = src == ref[idx]
    first = torch.full((N, F), E, dtype=torch.int64).scatter_reduce(
        0, idx.view(-1, 1).expand(E, F), torch.where(hit, e, torch.full_like(e, E)), "amin")
    assert torch.equal(arg, first)


def test_gather_forms_match_materialised_messages():
    g = torch.Generator().manual_seed(6)
    N, E, F = 200, 2500, 9
    x = torch.randn(N, F, generator=g)
    ei = torch.randint(N, (2, E), generator=g)
    w = torch.rand(E, generator=g)
    msg = w.view(-1, 1) * x[ei[0]]
    assert torch.equal(S.gather_sum(x, ei[0], ei[1], w, N), S.scatter_sum(msg, ei[1], N))
    o1, a1 = S.gather_max(x, ei[0], ei[1], N)
    o2, a2 = S.scatter_max(x[ei[0]], ei[1], N)
    assert torch.equal(o1, o2) and torch.equal(a1, a2)


def test_float64_twin_close():
    g = torch.Generator().manual_seed(7)
    N, E, F = 500, 6000, 8
    x = torch.randn(N, F, generator=g)
    ei = torch.randint(N, (2, E), generator=g)
    W = torch.randn(F, F, generator=g)
    o32 = P.gcn_conv(x, ei, W)
    o64 = P.gcn_conv(x.double(), ei, W.double())
    assert torch.allclose(o32.double(), o64, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", sorted(f for f in os.listdir(GOLDEN) if f.endswith(".npz"))
                         if os.path.isdir(GOLDEN) else [])
def test_golden_fixture_reproduces(name):
    from tests.golden import make_golden
    d = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    fresh = make_golden.compute(name[:-4], {k: d[k] for k in d.files})
    for k, v in fresh.items():
        assert np.array_equal(np.asarray(v), d[k]), (name, k)


def test_oracle_torch_scatter_documented_vectors():
    """torch_scatter 2.0.4 semantics on its documented small cases (1-D index
    along dim 0; empty segment -> 0 with arg = src.size(0); first index wins)."""
    from oracle import scatter_ref as S
    src = torch.tensor([1., 3, 2, 4, 5, 6])
    index = torch.tensor([0, 1, 0, 1, 1, 3])
    assert S.scatter_sum(src.view(-1, 1), index, 4).view(-1).tolist() == [3, 12, 0, 6]
    assert S.scatter_mean(src.view(-1, 1), index, 4).view(-1).tolist() == [1.5, 4, 0, 6]
    mn, amn = S.scatter_loop(src.view(-1, 1), index, 4, "min")
    mx, amx = S.scatter_loop(src.view(-1, 1), index, 4, "max")
    assert mn.view(-1).tolist() == [1, 3, 0, 6] and amn.view(-1).tolist() == [0, 1, 6, 5]
    assert mx.view(-1).tolist() == [2, 5, 0, 6] and amx.view(-1).tolist() == [2, 4, 6, 5]
    src2 = torch.tensor([[1., 2], [5, 6], [3, 4], [7, 8], [9, 10], [11, 12]])
    assert S.scatter_sum(src2, index, 4).tolist() == [[4, 6], [21, 24], [0, 0], [11, 12]]
    mx2, amx2 = S.scatter_loop(src2, index, 4, "max")
    assert mx2.tolist() == [[3, 4], [9, 10], [0, 0], [11, 12]] and amx2.tolist() == [[2, 2], [4, 4], [6, 6], [5, 5]]


def _dense(ei, w, N):
    """Operator of propagate(edge_index, norm) as a dense matrix: out = M x,
    M[i, j] = sum of the weights of edges j -> i (flow source_to_target)."""
    M = torch.zeros(N, N, dtype=torch.float64)
    for e in range(ei.shape[1]):
        M[ei[1, e], ei[0, e]] += w[e]
    return M


def _kat_graph():
    # 7 nodes: an undirected path 0-1-2-3, a triangle 3-4-5, a duplicate
    # edge (1->2 twice), a self loop on 4, node 6 isolated
    und = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 3)]
    src = [a for a, b in und] + [b for a, b in und] + [1, 4]
    dst = [b for a, b in und] + [a for a, b in und] + [2, 4]
    return torch.tensor([src, dst]), 7


@pytest.mark.parametrize("normalization", ["sym", "rw", None])
def test_kat_get_laplacian_and_cheb_conv(normalization):
    """The oracle's get_laplacian / ChebConv against the textbook operators
    built densely: L = D - A, I - D^-1/2 A D^-1/2, I - D^-1 A (degrees over
    edge_index[0] after removing loops), L_hat = 2 L / lambda_max - I, and
    the Chebyshev recursion T_0 = X, T_1 = L_hat X, T_k = 2 L_hat T_{k-1} - T_{k-2}."""
    ei, N = _kat_graph()
    keep = ei[0] != ei[1]
    A = torch.zeros(N, N, dtype=torch.float64)
    for s, d in ei[:, keep].t().tolist():
        A[d, s] += 1.0                   # message s -> d
    deg = torch.zeros(N, dtype=torch.float64)
    for s in ei[0, keep].tolist():
        deg[s] += 1.0                    # deg = scatter_add(w, row)
    I = torch.eye(N, dtype=torch.float64)
    if normalization is None:
        L = torch.diag(deg) - A
    elif normalization == "sym":
        dinv = torch.where(deg > 0, deg.pow(-0.5), torch.zeros_like(deg))
        L = I - dinv.view(-1, 1) * A * dinv.view(1, -1)
    else:
        # edge j -> i carries 1/deg[j] (deg of the source, edge_index[0])
        dinv = torch.where(deg > 0, 1.0 / deg, torch.zeros_like(deg))
        L = I - A * dinv.view(1, -1)
    lei, lw = P.get_laplacian(ei, None, normalization, torch.float64, N)
    assert torch.allclose(_dense(lei, lw, N), L, atol=1e-12)
    lam = 2.0 if normalization == "sym" else 3.5
    L_hat = 2.0 * L / lam - I
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, 3, generator=g, dtype=torch.float64)
    W = torch.randn(3, 3, 2, generator=g, dtype=torch.float64)
    b = torch.randn(2, generator=g, dtype=torch.float64)
    T = [x, L_hat @ x]
    T.append(2 * L_hat @ T[1] - T[0])
    want = sum(T[k] @ W[k] for k in range(3)) + b
    got = P.cheb_conv(x, ei, W, b, normalization=normalization, lambda_max=None if normalization == "sym" else lam)
    assert torch.allclose(got, want, atol=1e-12)
    # the propagated operator of cheb_norm is L_hat itself (the -I rides as separate loops)
    cei, cw = P.cheb_norm(ei, N, None, normalization, lam, torch.float64)
    assert torch.allclose(_dense(cei, cw, N), L_hat, atol=1e-12)
    assert cei.shape[1] == int(keep.sum()) + 2 * N      # edges, L's diagonal, the -1 loops


def test_kat_agnn_conv():
    """AGNNConv: x'_i = sum_{j in N(i) u {i}} softmax_j(beta cos(x_i, x_j)) x_j,
    with a duplicate edge counted twice and existing loops replaced by one."""
    ei, N = _kat_graph()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(N, 4, generator=g, dtype=torch.float64)
    beta = torch.tensor([0.7], dtype=torch.float64)
    xn = x / x.norm(dim=1, keepdim=True)
    want = torch.zeros_like(x)
    keep = ei[0] != ei[1]
    for i in range(N):
        srcs = [s for s, d in ei[:, keep].t().tolist() if d == i] + [i]
        sc = torch.stack([beta[0] * (xn[i] * xn[j]).sum() for j in srcs])
        p = torch.softmax(sc, 0)
        want[i] = sum(p[k] * x[j] for k, j in enumerate(srcs))
    assert torch.allclose(P.agnn_conv(x, ei, beta), want, atol=1e-12)


def test_kat_sg_conv_and_gin_conv():
    """SGConv = Linear(S^K X) with S = D^-1/2 (A + I) D^-1/2 (remaining loops:
    an existing loop keeps its weight), GINConv = nn((1 + eps) X + A X) with
    loops removed -- against dense operators."""
    ei, N = _kat_graph()
    keep = ei[0] != ei[1]
    A = torch.zeros(N, N, dtype=torch.float64)
    for s, d in ei[:, keep].t().tolist():
        A[d, s] += 1.0
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, 3, generator=g, dtype=torch.float64)
    Ah = A + torch.eye(N, dtype=torch.float64)
    deg = Ah.sum(0)                 # deg over edge_index[0] = column sums (sources)
    S_ = Ah / deg.sqrt().view(-1, 1) / deg.sqrt().view(1, -1)
    lw = torch.randn(2, 3, generator=g, dtype=torch.float64)
    lb = torch.randn(2, generator=g, dtype=torch.float64)
    want = (S_ @ (S_ @ x)) @ lw.t() + lb
    assert torch.allclose(P.sg_conv(x, ei, 2, lw, lb), want, atol=1e-12)
    mlp = torch.nn.Linear(3, 2).double()
    assert torch.allclose(P.gin_conv(x, ei, mlp, 0.25), mlp(1.25 * x + A @ x), atol=1e-12)


from hypothesis import HealthCheck, given, settings, strategies as st  # noqa: E402


@settings(max_examples=80, deadline=None, derandomize=True, database=None,
          suppress_health_check=[HealthCheck.too_slow])
@given(N=st.integers(1, 200), E=st.integers(0, 2000), F=st.integers(1, 9), ties=st.booleans(),
       seed=st.integers(0, 1 << 16))
def test_fuzz_oracle_forms_agree(N, E, F, ties, seed):
    """Property fuzzing of the oracle's two independent forms:
    torch's scatter_add_ / amax + first-hit amin vs the serial C loop
    (scatter_loop.c, torch_scatter's b/e/k loop), on empty inputs, empty
    rows and tie-heavy integer data."""
    g = torch.Generator().manual_seed(seed)
    src = (torch.randint(-2, 3, (E, F), generator=g).float() if ties else torch.randn(E, F, generator=g))
    idx = torch.randint(N, (E,), generator=g)
    assert torch.equal(S.scatter_sum(src, idx, N), S.scatter_loop(src, idx, N, "sum")[0])
    assert torch.equal(S.scatter_mean(src, idx, N), S.scatter_loop(src, idx, N, "mean")[0])
    for red, amax in (("max", "amax"), ("min", "amin")):
        out, arg = S.scatter_loop(src, idx, N, red)
        fill = float("-inf") if red == "max" else float("inf")
        ref = torch.full((N, F), fill).scatter_reduce(0, idx.view(-1, 1).expand(E, F), src, amax)
        empty = torch.isinf(ref)
        ref[empty] = 0
        assert torch.equal(out, ref)
        e = torch.arange(E).view(-1, 1).expand(E, F)
        hit = src == ref[idx]
        first = torch.full((N, F), E, dtype=torch.int64).scatter_reduce(
            0, idx.view(-1, 1).expand(E, F), torch.where(hit, e, torch.full_like(e, E)), "amin")
        first[empty] = E
        assert torch.equal(arg, first)


@pytest.mark.parametrize("reduce", ["sum", "mean", "max", "min"])
def test_any_dtype_loop_matches_c_loop_and_kats(reduce):
    """scatter_loop_any (the numpy restatement used for float64 / float16 /
    int64) equals the C serial loop on float32, tie-heavy data included, and
    hand-computed int64 KATs (truncating mean, lowest() -> 0, first-index arg)."""
    g = torch.Generator().manual_seed(11)
    src = torch.randint(-3, 4, (700, 6), generator=g).float()
    idx = torch.randint(60, (700,), generator=g)
    a, b = S.scatter_loop(src, idx, 64, reduce)
    c, d = S.scatter_loop_any(src, idx, 64, reduce)
    assert torch.equal(a, c) and (b is None or torch.equal(b, d))
    lo = torch.iinfo(torch.int64).min
    s = torch.tensor([[-7], [2], [lo], [5], [5]], dtype=torch.int64)
    i = torch.tensor([0, 0, 1, 2, 2])
    o, arg = S.scatter_loop_any(s, i, 4, reduce)
    want = {"sum": ([-5], [lo], [10], [0]), "mean": ([-2], [lo], [5], [0]),
            "max": ([2], [0], [5], [0]), "min": ([-7], [lo], [5], [0])}[reduce]
    assert o.view(-1).tolist() == [w[0] for w in want]
    if arg is not None:
        # max: lowest() itself never beats the init value (arg stays E = 5, value -> 0)
        assert arg.view(-1).tolist() == ([1, 5, 3, 5] if reduce == "max" else [0, 2, 3, 5])


def test_gat_dropout_keep_hash_restatement():
    """oracle.pyg_ref.gat_dropout_keep_slots (numpy, vectorised) against a
    plain-int restatement of csrc/mp_agg.h drop_hash, including a seed
    with high bits and slot*H + h past 2^32; keep fraction ~ 1 - p; the oracle
    layer with an all-keep mask scales the messages by 1/(1-p)."""
    M = 0xFFFFFFFF

    def mix(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & M
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & M
        return h ^ (h >> 16)

    def keep(seed, p, idx):
        a = mix((idx & M) ^ (seed & M))
        b = mix((a + 0x9E3779B9 * (((idx >> 32) ^ (seed >> 32)) & M) + 0x632BE5AB) & M)
        return b >= min(int(np.floor(float(np.float32(p)) * 4294967296.0)), M)

    for seed, p, H, n in ((0, 0.5, 1, 300), (0xDEADBEEF12345678, 0.3, 8, 200), (2 ** 64 - 1, 0.9, 3, 100)):
        got = P.gat_dropout_keep_slots(seed, p, H, n)
        want = torch.tensor([[keep(seed, p, s * H + h) for h in range(H)] for s in range(n)])
        assert torch.equal(got, want)
    # indices past 2^32 (the high word enters the second round)
    seed, H = 99, 8
    big = (1 << 32) // H + 5
    got = P.gat_dropout_keep_slots(seed, 0.4, H, 3, start=big - 3)
    want = torch.tensor([[keep(seed, 0.4, s * H + h) for h in range(H)] for s in range(big - 3, big)])
    assert torch.equal(got, want)
    frac = P.gat_dropout_keep_slots(5, 0.3, 4, 50000).float().mean().item()
    assert abs(frac - 0.7) < 0.005
    g = torch.Generator().manual_seed(3)
    N, H, C = 30, 2, 4
    x = torch.randn(N, 5, generator=g, dtype=torch.float64)
    ei = torch.randint(0, N, (2, 120), generator=g)
    W = torch.randn(5, H * C, generator=g, dtype=torch.float64)
    att = torch.randn(1, H, 2 * C, generator=g, dtype=torch.float64)
    E = P.add_self_loops(P.remove_self_loops(ei)[0], num_nodes=N)[0].shape[1]
    a = P.gat_conv(x, ei, W, att, None, H, C)
    b = P.gat_conv(x, ei, W, att, None, H, C, drop_keep=torch.ones(E, H, dtype=torch.bool), drop_p=0.25)
    assert torch.allclose(b, a / (1 - float(np.float32(0.25))), rtol=1e-12, atol=1e-12)


def test_kat_composites_against_per_segment_float64():
    """The oracle's torch_scatter composites (softmax, log_softmax, logsumexp,
    std) against a float64 per-segment evaluation of their formulas, with an
    empty segment and a one-element segment."""
    g = torch.Generator().manual_seed(4)
    idx = torch.tensor([0, 2, 0, 2, 3, 2, 0, 5])
    src = torch.randn(8, 3, generator=g)
    n = 6
    sm = S.scatter_softmax(src, idx)
    lsm = S.scatter_log_softmax(src, idx)
    lse = S.scatter_logsumexp(src, idx, n)
    sd = S.scatter_std(src, idx, n)
    sdb = S.scatter_std(src, idx, n, unbiased=False)
    for r in range(n):
        m = idx == r
        if not bool(m.any()):
            assert bool(torch.isinf(lse[r]).all()) and bool((lse[r] < 0).all())
            assert torch.equal(sd[r], torch.zeros(3))
            continue
        x = src[m].double()
        e = (x - x.max(0).values).exp()
        assert torch.allclose(sm[m].double(), e / (e.sum(0) + 1e-12), atol=1e-6)
        assert torch.allclose(lsm[m].double(), (x - x.max(0).values) - torch.log(e.sum(0) + 1e-12), atol=1e-6)
        assert torch.allclose(lse[r].double(), torch.log(e.sum(0) + 1e-12) + x.max(0).values, atol=1e-6)
        c = x.shape[0]
        dev2 = ((x - x.mean(0)) ** 2).sum(0)
        assert torch.allclose(sd[r].double(), (dev2 / (max(c - 1, 1) + 1e-6)).sqrt(), atol=1e-5)
        assert torch.allclose(sdb[r].double(), (dev2 / (c + 1e-6)).sqrt(), atol=1e-5)
