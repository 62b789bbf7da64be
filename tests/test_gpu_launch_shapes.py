"""Launch shapes the rest of the suite never reaches: code paths that only the
input SIZE or an ABI flag selects.

  A. mp_gemm_rows_f32: the persistent MFMA kernel with more than one tile per
     workgroup, trans_w = 1, every host dispatch condition, ldc > N, and that
     nothing outside [M, N] is written.
  C. one call past the grid cap of each capped grid-stride kernel, so the
     loop body runs a second time (and ends on a partial block).
(B, the spline block shapes, extends tests/test_gpu_spline.py in place.)

Exactness.  "Integer data" is integers in [-8, 8] stored as fp32: every
product is an integer of magnitude <= 64 and every partial sum of the k-ordered
fmaf chain an integer of magnitude <= 64 K (16384 for K = 256) < 2^24, so the
chain is exact and must equal the float64 product cast to float BITWISE.  Random
data is checked bitwise between code paths and against float64 under the bound
of test_gemm_rows_row_exact, 1e-5 * max(1, sum |x w|).  Everything in C is
bitwise against a reference the suite already has.
"""
import pytest
import torch

from oracle import scatter_ref as S
from oracle import pyg_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
CAP_ROWS = 262144                     # 65536 blocks x 4 waves: k_seg_any, k_segment_sum_serial, k_arg_bwd_csr
N_PAST = CAP_ROWS + 777               # the second pass of the loop ends on a partial block


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _int_pair(M, K, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-8, 9, (M, K), generator=g).float()
    w = torch.randint(-8, 9, (K, N), generator=g).float()
    return x.to(DEV), w.to(DEV)


def _rand_pair(M, K, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(K, N, generator=g) / K ** 0.5
    return x.to(DEV), w.to(DEV)


def _f64(x, w):
    """The float64 product cast to float: the exact result on integer data."""
    return (x.double() @ w.double()).float()


def _assert_float64_bound(got, x, w):
    ref = x.double() @ w.double()
    bound = 1e-5 * (x.abs().double() @ w.abs().double()).clamp(min=1.0)
    err = (got.double() - ref).abs()
    print("max |err| / bound = %.3g" % float((err / bound).max()))
    assert (err <= bound).all()


def _gemm_direct(x, w_stored, N, trans_w=0, force_generic=0, pad_rows=0, pad_cols=0, sentinel=None):
    """mp_gemm_rows_f32 through the C-ABI: w_stored is [K, N] (trans_w = 0) or
    [N, K] (trans_w = 1), both contiguous.  The output buffer is [M + pad_rows,
    N + pad_cols] with ldc = N + pad_cols, filled with `sentinel` first."""
    from mi355_mp import _lib
    M, K = x.shape
    assert w_stored.is_contiguous() and tuple(w_stored.shape) == ((N, K) if trans_w else (K, N))
    assert x.stride(1) == 1
    buf = torch.empty((M + pad_rows, N + pad_cols), dtype=torch.float32, device=x.device)
    if sentinel is not None:
        buf.fill_(sentinel)
    _lib.check(_lib.load().mp_gemm_rows_f32(x.data_ptr(), x.stride(0), M, K, w_stored.data_ptr(), trans_w, N,
                                            buf.data_ptr(), buf.stride(0), force_generic,
                                            _lib.stream_ptr(x.device)), "mp_gemm_rows_f32")
    return buf


def _assert_mfma_multi_tile(x, w, cu):
    """The dispatch conditions of the MFMA kernel (csrc/mp_gemm.hip), and more
    than one 64-row tile for every persistent workgroup: asserted, so the test
    cannot silently run the generic kernel or a single loop iteration."""
    assert x.dtype == torch.float32 and x.is_contiguous()
    assert x.shape[1] == 256 and tuple(w.shape) == (256, 256)
    assert x.data_ptr() % 16 == 0 and x.stride(0) % 4 == 0 and 64 * x.stride(0) < 2 ** 32 - 1
    assert x.shape[0] > 64 * cu


# A.1 the persistent multi-tile MFMA path --------------------------------------------

def _multi_tile_m(cu):
    # 2 cu + 2 tiles on cu workgroups: workgroups 0 and 1 run three tiles, the
    # rest two; the globally last tile (tile 2 cu + 1, 37 rows) is the third of workgroup 1
    return 64 * (2 * cu + 1) + 37


@pytest.fixture(scope="module")
def multi_int():
    cu = _cu()
    x, w = _int_pair(_multi_tile_m(cu), 256, 256, 11)
    return cu, x, w, _f64(x, w)


@pytest.fixture(scope="module")
def multi_rand():
    cu = _cu()
    x, w = _rand_pair(_multi_tile_m(cu), 256, 256, 12)
    return cu, x, w


def test_gemm_mfma_multi_tile_integer_data_bitwise(multi_int):
    """k_gemm_n256 re-entering its persistent loop (the double-buffered LDS
    image, the prefetch of tile t + gridDim.x, the deferred store of the
    previous tile's C, the buffer flip), on integer data: bitwise the float64
    product on every row -- a wrong tile, a stale buffer or a misplaced row
    cannot hide in rounding."""
    from mi355_mp import ops
    cu, x, w, ref = multi_int
    _assert_mfma_multi_tile(x, w, cu)
    n_tiles = (x.shape[0] + 63) // 64
    print("cu = %d, M = %d, tiles = %d (%d workgroups: %d with three tiles, the rest two)"
          % (cu, x.shape[0], n_tiles, cu, n_tiles - 2 * cu))
    assert n_tiles == 2 * cu + 2 and x.shape[0] % 64 == 37
    got = ops.gemm_rows(x, w)
    assert torch.equal(got, ref), int((got != ref).any(dim=1).sum())
    assert torch.equal(ops.gemm_rows(x, w), got)                      # and repeatable


def test_gemm_mfma_multi_tile_random_data(multi_rand):
    """The same launch on random data: bitwise the generic kernel, bitwise row
    for row calls on slices that span a workgroup's tile boundaries (one tile
    per workgroup there, or again several), and inside the float64 bound."""
    from mi355_mp import ops
    cu, x, w = multi_rand
    _assert_mfma_multi_tile(x, w, cu)
    M = x.shape[0]
    full = ops.gemm_rows(x, w)
    assert torch.equal(ops.gemm_rows(x, w, force_generic=True), full)
    for a, b in ((64 * cu - 3, 64 * cu + 70), (64 * 2 * cu + 5, M), (64 * cu - 3, M), (0, 64 * cu + 1), (1, M)):
        assert x[a:b].data_ptr() % 16 == 0
        assert torch.equal(ops.gemm_rows(x[a:b], w), full[a:b]), (a, b)
    _assert_float64_bound(full, x, w)


# A.2 padding and overrun -----------------------------------------------------------

@pytest.mark.parametrize("path", ["mfma", "generic"])
def test_gemm_writes_nothing_outside_m_by_n(path):
    """ldc = N + 4 and 64 spare rows, all holding a sentinel: rows < M and
    columns < N are ops.gemm_rows' result, every other element is untouched
    (the partial last tile's rows >= M are 'loaded, never stored')."""
    from mi355_mp import ops
    cu = _cu()
    M, K, N = (64 * cu + 37, 256, 256) if path == "mfma" else (100, 24, 64)
    x, w = _rand_pair(M, K, N, 21)
    if path == "mfma":
        _assert_mfma_multi_tile(x, w, cu)
    sentinel = -12345.75
    buf = _gemm_direct(x, w, N, pad_rows=64, pad_cols=4, sentinel=sentinel)
    assert buf.stride(0) == N + 4
    assert torch.equal(buf[:M, :N], ops.gemm_rows(x, w))
    assert torch.equal(buf[:M, :N], ops.gemm_rows(x, w, force_generic=True))
    rest = buf.clone()
    rest[:M, :N] = sentinel
    assert torch.equal(rest, torch.full_like(rest, sentinel)), int((rest != sentinel).sum())


# A.3 trans_w = 1 -------------------------------------------------------------------

def test_gemm_trans_w_mfma_multi_tile(multi_int):
    """C = A W^T with W stored [N, K] (BT = true of k_gemm_n256), at the
    multi-tile M on integer data: bitwise the float64 product, and the generic
    kernel's BT = true form bitwise the same."""
    cu, x, w, ref = multi_int
    _assert_mfma_multi_tile(x, w, cu)
    wt = w.t().contiguous()                                           # [N, K]: A wt^T = A w
    got = _gemm_direct(x, wt, 256, trans_w=1)
    assert torch.equal(got, ref), int((got != ref).any(dim=1).sum())
    assert torch.equal(_gemm_direct(x, wt, 256, trans_w=1, force_generic=1), got)


@pytest.mark.parametrize("K,N", [(24, 64), (50, 1000), (17, 65), (1, 1), (16, 64)])
def test_gemm_trans_w_generic(K, N):
    """BT = true of k_gemm_rows: integer data bitwise against float64; random
    data bitwise ops.gemm_rows on the transposed copy (the fmaf chain over k is
    the same whichever way W is read)."""
    from mi355_mp import ops
    M = 131
    x, w = _int_pair(M, K, N, K * 7 + N)
    assert torch.equal(_gemm_direct(x, w.t().contiguous(), N, trans_w=1), _f64(x, w))
    x, w = _rand_pair(M, K, N, K * 7 + N + 1)
    wt = w.t().contiguous()                                           # W as stored: [N, K]
    assert torch.equal(_gemm_direct(x, wt, N, trans_w=1), ops.gemm_rows(x, wt.t().contiguous()))


# A.4 dispatch conditions -----------------------------------------------------------

def test_gemm_dispatch_conditions():
    """K = N = 256, M = 200: every way the host wrapper picks (or refuses) the
    MFMA kernel gives bitwise the contiguous call's rows."""
    from mi355_mp import ops
    M = 200
    x, w = _rand_pair(M, 256, 256, 31)
    want = ops.gemm_rows(x, w)
    assert torch.equal(ops.gemm_rows(x, w, force_generic=True), want)

    def view_of(cols, lo):
        buf = torch.full((M, cols), float("nan"), device=DEV)
        buf[:, lo:lo + 256] = x
        return buf[:, lo:lo + 256]

    v = view_of(260, 0)                                               # lda = 260 > K: still MFMA
    assert v.stride(0) == 260 and v.data_ptr() % 16 == 0
    assert torch.equal(ops.gemm_rows(v, w), want)
    v = view_of(260, 1)                                               # A not 16-byte aligned: generic
    assert v.stride(0) == 260 and v.data_ptr() % 16 == 4
    assert torch.equal(ops.gemm_rows(v, w), want)
    v = view_of(257, 0)                                               # lda % 4 != 0: generic
    assert v.stride(0) == 257
    assert torch.equal(ops.gemm_rows(v, w), want)
    v = x.t().contiguous().t()                                        # inner stride != 1: the wrapper's .contiguous()
    assert v.stride(1) != 1 and torch.equal(v, x)
    assert torch.equal(ops.gemm_rows(v, w), want)
    # two rows 2^26 floats apart: 64 * lda >= 2^32, the generic kernel's 64-bit row addressing
    lda = 2 ** 26
    big = torch.empty(lda + 256, device=DEV)
    v = torch.as_strided(big, (2, 256), (lda, 1))
    v.copy_(x[:2])
    assert v.stride(0) == lda and 64 * v.stride(0) >= 2 ** 32 and v.data_ptr() % 16 == 0
    assert torch.equal(ops.gemm_rows(v, w), want[:2])
    del big, v


# A.5 generic kernel edges ------------------------------------------------------------

@pytest.mark.parametrize("K,N", [(1, 1), (3, 5), (16, 64), (17, 65)])
def test_gemm_generic_edge_shapes(K, N):
    """k_gemm_rows at the tile edges the existing grid skips (one k, exactly one
    16-row k-step and 64-column tile, one past both), M = 131 (three row tiles,
    the last with 3 rows)."""
    from mi355_mp import ops
    M = 131
    x, w = _int_pair(M, K, N, K * 7 + N)
    assert torch.equal(ops.gemm_rows(x, w), _f64(x, w))
    x, w = _rand_pair(M, K, N, K * 7 + N + 1)
    full = ops.gemm_rows(x, w)
    _assert_float64_bound(full, x, w)
    for a, b in ((0, 1), (5, 70), (64, 128), (63, 131), (130, 131)):
        assert torch.equal(ops.gemm_rows(x[a:b], w), full[a:b]), (a, b)
        assert torch.equal(ops.gemm_rows(x[a:b].clone(), w), full[a:b]), (a, b)


# C. one call past each grid cap ---------------------------------------------------

@pytest.fixture(scope="module")
def hub_index():
    """E = 400000 rows of a scatter into N_PAST segments: row 7 is a hub (1/8 of
    the edges), the last 1000 segments stay empty."""
    E = 400_000
    g = torch.Generator().manual_seed(41)
    idx = torch.cat([torch.full((E // 8,), 7, dtype=torch.int64),
                     torch.randint(N_PAST - 1000, (E - E // 8,), generator=g)])
    idx = idx[torch.randperm(E, generator=g)]
    assert int(idx.max()) < N_PAST - 1000
    return idx


@pytest.mark.parametrize("dtype", [torch.float64, torch.int64])
@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_segment_reduce_past_the_row_cap(hub_index, dtype, reduce):
    """k_seg_any over 262144 + 777 rows (grid capped at 65536 blocks of four
    rows): values and first-edge args bitwise the serial-loop oracle.  As the
    index leaves the last 1000 rows empty, the mirrored index N - 1 - idx is
    run too: it puts the hub and populated rows in the loop's second pass, and
    its reference is the same oracle result with the rows reversed (the order
    of the edges within a row does not change)."""
    import torch_scatter
    idx, N, F = hub_index, N_PAST, 3
    E = idx.numel()
    g = torch.Generator().manual_seed(42)
    if dtype == torch.int64:
        src = torch.randint(-50, 50, (E, F), generator=g)
    else:
        src = torch.randint(-40, 40, (E, F), generator=g).double() * 0.37 + torch.rand(E, F, generator=g).double()
    ref, rarg = S.scatter_loop_any(src, idx, N, reduce)
    fn = getattr(torch_scatter, "scatter_" + reduce)
    for mirrored in (False, True):
        index = (N - 1 - idx) if mirrored else idx
        res = fn(src.to(DEV), index.to(DEV), 0, dim_size=N)
        out, arg = (res if isinstance(res, tuple) else (res, None))
        assert out.dtype == dtype and out.shape == (N, F)
        assert torch.equal(out.cpu(), ref.flip(0) if mirrored else ref), mirrored
        if reduce == "max":
            assert torch.equal(arg.cpu(), rarg.flip(0) if mirrored else rarg), mirrored
    # plain: every row of the second pass is empty (written as 0); mirrored: the hub and ~700 populated rows
    assert float(ref[CAP_ROWS:].abs().max()) == 0 and int((ref[:N - CAP_ROWS] != 0).any(dim=1).sum()) > 300


def test_weighted_gcn_degree_past_the_row_cap():
    """k_segment_sum_serial over 262144 + 777 source rows: GCNConv.norm with
    real-valued weights bit-equal to the oracle's edge-order scatter_add; one
    source has 5000 out-edges, sources on both sides of the cap have edges."""
    from torch_geometric.nn.conv.gcn_conv import GCNConv
    N, E = N_PAST, 500_000
    g = torch.Generator().manual_seed(43)
    src = torch.cat([torch.full((5_000,), N - 5, dtype=torch.int64), torch.randint(N, (E - 5_000,), generator=g)])
    ei = torch.stack([src, torch.randint(N, (E,), generator=g)])
    ei = ei[:, torch.randperm(E, generator=g)].contiguous()
    w = torch.rand(E, generator=g) * 3
    e1, n1 = GCNConv.norm(ei.to(DEV), N, w.to(DEV), False)
    r_ei, r_norm = P.gcn_norm(ei, N, w, False)
    assert torch.equal(e1.cpu(), r_ei)
    assert torch.equal(n1.cpu(), r_norm), float((n1.cpu() - r_norm).abs().max())


def _arg_backward_reference(arg, g, src, w, n_src):
    """As in tests/test_gpu_parity.py: torch_scatter's ScatterMax.backward then
    the message's and index_select's backward on the CPU, sequential in edge order."""
    E = src.numel()
    F = g.shape[1]
    gm = torch.zeros(E + 1, F).scatter_(0, arg, g)[:E]
    if w is not None:
        gm = gm * w.view(-1, 1)
    return torch.zeros(n_src, F).index_add_(0, src, gm)


def test_weighted_max_backward_past_the_row_cap():
    """k_arg_bwd_csr over a transposed CSR of 262144 + 777 source rows: d x of a
    weighted max bit-equal to the reference's edge-order index_add_.  Tie-heavy
    integer x with duplicate edges (the first edge wins), one source with 5000
    out-edges beyond the cap, and sources without out-edges on both sides of it
    (their rows must come back zero: the buffer is not cleared first)."""
    from mi355_mp import ops
    from mi355_mp.graph import Graph
    N, E, F = N_PAST, 500_000, 3
    g = torch.Generator().manual_seed(44)
    src = torch.cat([torch.full((5_000,), N - 9, dtype=torch.int64), torch.randint(N, (E - 5_000,), generator=g)])
    ei = torch.stack([src, torch.randint(N, (E,), generator=g)])
    ei = ei[:, torch.randperm(E, generator=g)].contiguous()
    x = torch.randint(-3, 4, (N, F), generator=g).float()
    w = torch.tensor([0.5, 1.0, 2.0, 0.75])[torch.randint(4, (E,), generator=g)]
    gout = torch.randn(N, F, generator=g)
    graph = Graph(ei.to(DEV), N, N)
    xd = x.to(DEV).requires_grad_(True)
    out = ops.fused_propagate(graph, xd, ei.to(DEV), w.to(DEV), "max")
    out.backward(gout.to(DEV))
    ref_out, arg = S.scatter_loop(x[ei[0]] * w.view(-1, 1), ei[1], N, "max")
    assert torch.equal(out.detach().cpu(), ref_out)
    gx_ref = _arg_backward_reference(arg, gout, ei[0], w, N)
    got = xd.grad.cpu()
    assert torch.equal(got, gx_ref), float((got - gx_ref).abs().max())
    deg = torch.bincount(ei[0], minlength=N)
    assert int((deg[CAP_ROWS:] == 0).sum()) > 0 and float(gx_ref[CAP_ROWS:].abs().max()) > 0


@pytest.mark.parametrize("F", [8, 5])
def test_gather_rows_f32_past_the_row_cap(F):
    """k_gather_rows<4> (F = 8) and <1> (F = 5) with 40000 indices, past the
    32768 rows of the capped grid: bitwise x[idx]."""
    from mi355_mp import ops
    g = torch.Generator().manual_seed(45 + F)
    x = torch.randn(5000, F, generator=g).to(DEV)
    idx = torch.randint(5000, (40_000,), generator=g).to(DEV)
    assert x.data_ptr() % 16 == 0
    assert torch.equal(ops.gather_rows(x, idx), x[idx])


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.float64])
@pytest.mark.parametrize("F", [8, 5])
def test_gather_rows_any_past_the_row_cap(dtype, F):
    """k_gather_any for 2-, 4- and 8-byte elements with 70000 indices, past the
    65536 rows of the capped grid: bitwise x[idx].  ops.gather_rows sends
    float16 and float64 there; float32 goes to mp_gather_rows_f32 from every
    ops entry, so the 4-byte form is called through the C-ABI directly."""
    from mi355_mp import _lib, ops
    g = torch.Generator().manual_seed(47 + F)
    x = (torch.randint(-2000, 2000, (5000, F), generator=g).double() * 0.25).to(dtype).to(DEV)
    idx = torch.randint(5000, (70_000,), generator=g).to(DEV)
    if dtype == torch.float32:
        out = torch.full((idx.numel(), F), float("nan"), device=DEV)
        _lib.check(_lib.load().mp_gather_rows_any(4, x.data_ptr(), x.stride(0), idx.data_ptr(), idx.numel(), F,
                                                  out.data_ptr(), out.stride(0), _lib.stream_ptr(x.device)),
                   "mp_gather_rows_any")
    else:
        out = ops.gather_rows(x, idx)
    assert out.dtype == dtype and torch.equal(out, x[idx])
