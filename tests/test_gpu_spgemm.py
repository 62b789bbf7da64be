"""torch_sparse.spspmm / ops.spgemm against the dense float64 product: exact indices (so sorted and
coalesced), values within 1e-5 * sum |terms|, bitwise for small integers, the same bits on a second
run.  Shapes sit on both sides of every bin limit mp_spgemm_bin_cap reports."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _coo(d):
    idx = d.nonzero().t().contiguous()
    return idx, d[idx[0], idx[1]].float()


def _ints(g, *shape, density=1.0):
    v = torch.randint(1, 4, shape, generator=g).double() * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    return v * (torch.rand(shape, generator=g) < density)


def _two_slot_row(ub, g):
    # B's row 0 holds ub - 7 entries, row 1 holds 7 that overlap them: A's row 0 has that ub
    A = torch.tensor([[2.0, 3.0], [0.0, 1.0]], dtype=torch.float64)
    B = torch.zeros(2, ub + 3, dtype=torch.float64)
    B[0, 5:ub - 2] = _ints(g, ub - 7)
    B[1, 1:8] = _ints(g, 7)
    return A, B


def _case(name):
    # -> (A, B dense float64, drop flag)
    from mi355_mp import ops
    g = torch.Generator().manual_seed(len(name))
    cap = ops.spgemm_bin_cap
    if name == "empty":
        return torch.zeros(4, 3, dtype=torch.float64), torch.zeros(3, 5, dtype=torch.float64), False
    if name == "no_products":                       # A reaches only B's empty rows
        A, B = torch.zeros(6, 4, dtype=torch.float64), torch.zeros(4, 6, dtype=torch.float64)
        A[:, 0], B[1] = _ints(g, 6), _ints(g, 6)
        return A, B, False
    if name == "rectangular":
        return _ints(g, 5, 7, density=0.6), _ints(g, 7, 3, density=0.6), False
    if name == "continuous":                        # away from 0: the structural mask stays exact
        A = (torch.rand(70, 90, generator=g, dtype=torch.float64) + 0.5) * _ints(g, 70, 90, density=0.2).sign()
        B = (torch.rand(90, 300, generator=g, dtype=torch.float64) + 0.5) * _ints(g, 90, 300, density=0.1).sign()
        return A.float().double(), B.float().double(), False
    if name == "one_column":                        # 50 products of a row on one column
        A, B = torch.zeros(2, 50, dtype=torch.float64), torch.zeros(50, 9, dtype=torch.float64)
        A[0], B[:, 3] = _ints(g, 50), _ints(g, 50)
        return A, B, False
    if name == "probing":                           # a row's columns all congruent modulo the table size
        slots = cap("wave_slots")
        A, B = _ints(g, 1, 2), torch.zeros(2, 10 * slots, dtype=torch.float64)
        B[0, ::slots], B[1, slots::2 * slots] = _ints(g, 10), _ints(g, 5)
        return A, B, False
    if name.startswith("ub_"):                      # ub_<bin>_<-1|0|1>
        _, which, d = name.split("_")
        return _two_slot_row(cap(which) + int(d), g) + (False,)
    if name == "star":                              # (A + I)^2 of a star: the hub row in the window bin
        n = cap("workgroup") // 3 + 200
        S = torch.eye(n, dtype=torch.float64)
        S[0, :] = S[:, 0] = 1
        return S, S, False
    if name == "windows":                           # a row over three windows, the last one partial
        n = 2 * cap("window") + 37
        A = _ints(g, 3, 40)
        B = _ints(g, 40, n, density=3 * cap("workgroup") / (40 * n))       # ub = 3 caps a row
        B[:, cap("window") - 1:cap("window") + 1] = 1      # both sides of a window's edge
        B[:, n - 1] = 2
        return A, B, False
    if name == "drop_diagonal":                     # row 5's only entry is its diagonal
        A, B = _ints(g, 30, 30, density=0.2), _ints(g, 30, 30, density=0.2)
        A[5], B[2] = 0, 0
        A[5, 2] = B[2, 5] = 1
        return A, B, True
    raise KeyError(name)


def _run(idx_a, val_a, idx_b, val_b, m, k, n, drop):
    from mi355_mp import ops
    import torch_sparse
    dev = torch.device("cuda:0")
    args = (idx_a.to(dev), val_a.to(dev), idx_b.to(dev), val_b.to(dev), m, k, n)
    if drop:
        i, v = ops.spgemm(*args, drop_diagonal=True)
    else:
        i, v = torch_sparse.spspmm(*args)
    assert i.dtype == torch.int64 and v.dtype == torch.float32 and i.shape == (2, v.numel())
    return i.cpu(), v.cpu()


def _check(A, B, operands, drop, exact):
    m, k, n = A.shape[0], A.shape[1], B.shape[1]
    idx, val = _run(*operands, m, k, n, drop)
    mask = ((A != 0).double() @ (B != 0).double()) > 0
    if drop:
        mask &= ~torch.eye(m, n, dtype=torch.bool)
    want = mask.nonzero().t()
    assert torch.equal(idx, want), (idx.shape, want.shape)
    ref = (A @ B)[want[0], want[1]]
    bound = 1e-5 * (A.abs() @ B.abs())[want[0], want[1]]
    err = (val.double() - ref).abs()
    assert bool((err <= bound).all())
    if exact:
        assert torch.equal(val, ref.float())
    idx2, val2 = _run(*operands, m, k, n, drop)
    assert torch.equal(idx, idx2) and torch.equal(val.view(torch.int32), val2.view(torch.int32))


CASES = ["empty", "no_products", "rectangular", "continuous", "one_column", "probing", "star", "windows",
         "drop_diagonal"] + ["ub_%s_%d" % (b, d) for b in ("wave", "workgroup") for d in (-1, 0, 1)]


@pytest.mark.parametrize("name", CASES)
def test_spspmm_matches_the_dense_product(name):
    A, B, drop = _case(name)
    _check(A, B, _coo(A) + _coo(B), drop, exact=name != "continuous")


def test_unsorted_inputs_with_duplicates():
    """Entries in random order, a third of them repeated: a duplicate counts as its sum (positive values,
    so no operand entry cancels and the mask stays exact)."""
    g = torch.Generator().manual_seed(7)
    ops_, dense = [], []
    for rows, cols, nnz in ((40, 60, 500), (60, 80, 700)):
        idx = torch.stack([torch.randint(0, rows, (nnz,), generator=g), torch.randint(0, cols, (nnz,), generator=g)])
        idx = torch.cat([idx, idx[:, :nnz // 3]], dim=1)[:, torch.randperm(nnz + nnz // 3, generator=g)]
        val = torch.randint(1, 4, (idx.shape[1],), generator=g).float()
        ops_ += [idx, val]
        dense.append(torch.zeros(rows, cols, dtype=torch.float64).index_put_((idx[0], idx[1]), val.double(),
                                                                             accumulate=True))
    _check(dense[0], dense[1], tuple(ops_), False, exact=True)


def test_products_that_cancel_keep_their_entry():
    idx, val = _run(torch.tensor([[0, 0], [0, 1]]), torch.tensor([1.0, -1.0]), torch.tensor([[0, 1], [0, 0]]),
                    torch.tensor([1.0, 1.0]), 1, 2, 1, False)
    assert idx.tolist() == [[0], [0]] and val.tolist() == [0.0]

