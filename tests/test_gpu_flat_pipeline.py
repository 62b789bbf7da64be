"""The rolling gather window of k_agg_flat's scalar-batch path, on small graphs.

Where x lies beyond the Infinity Cache the kernel keeps a ring of R = 4 gathers
full from a task's first slot to its last batch (csrc/mp_flat_ring.h); the
other instances issue and consume batches of 8 or 16 whole.  Either way, what
can go wrong sits where a task, a row or a batch ends.  The graphs here are built row by row against the merge-path
schedule (task = `chunk` units, a row marker and a slot one unit each) so that
tasks of every critical length exist -- 1, R - 1, R, R + 1, 2R - 1, 2R + 1 slots
for batches of 4, 8 and 16 -- next to rows that end on a batch boundary, tasks
that continue a row for fewer slots than a batch, runs of empty rows longer
than the 64-row window (inside a task and across task ends), split hub rows
and a final task whose batches reach the end of the arrays.  What the schedule
really holds is read back and asserted, not assumed.

Expected: rows summed by one task bitwise equal to the serial loop of
oracle.scatter_ref, split rows within 1e-5 * sum|terms|, two runs bitwise
equal.  F = 64, 100 (4 features per lane), 128, 256; sum and mean; with and
without weights and bias; the far instance (the ring) and the near one; task
counts around one block and around a multiple of 8 blocks."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import scatter_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHUNK = 64


def _mods():
    from mi355_mp import _lib, ops
    from mi355_mp.graph import CSR
    return _lib, ops, CSR


class _tuned:
    def __init__(self, **kv):
        from mi355_mp import _lib
        self.lib = _lib.load()
        self.kv = {getattr(_lib, "MP_TUNE_" + k.upper()): v for k, v in kv.items()}
        self.prev = {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.prev[k] = self.lib.mp_tune(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            self.lib.mp_tune(k, v)
        return False


LENGTHS = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33)   # 1, R - 1, R, R + 1, 2R - 1, 2R + 1 for R = 4, 8, 16


def _degrees(chunk=CHUNK, seed=0, filler=400):
    """Row degrees of the test graph, built against the schedule: `pos` is the
    unit position (row markers + slots so far); tasks start at multiples of
    chunk, except where a start inside a row of <= chunk/2 slots snaps back."""
    rng = np.random.RandomState(seed)
    deg = []

    def pos():
        return len(deg) + int(sum(deg))

    def align():
        while pos() % chunk:
            deg.append(0)

    # a task of exactly L slots: chunk - L row markers share it
    for L in LENGTHS:
        align()
        rows = chunk - L
        head = [(L + 1) // 2, L // 2]
        deg.extend(head + [0] * (rows - 2))
    # a split hub row whose last task continues it for k < 8 slots, then > 64 empty rows
    for k in (1, 3, 7):
        align()
        deg.append(3 * chunk - 1 + k)       # its marker and slots end k units into the fourth task
        assert pos() % chunk == k, (pos(), k)
        deg.extend([0] * 150)               # the row window (64 rows) refills in the tasks that follow
    # rows that end exactly 8 and 16 slots into a task
    for first in (8, 16, 24, 32):
        align()
        deg.extend([first, 5, 0, 3])
    # filler: short rows, empty runs, a few hubs
    for _ in range(filler):
        t = rng.rand()
        if t < 0.45:
            deg.append(int(rng.randint(0, 4)))
        elif t < 0.8:
            deg.append(int(rng.randint(4, 40)))
        elif t < 0.9:
            deg.extend([0] * int(rng.randint(1, 90)))
        else:
            deg.append(int(rng.randint(100, 900)))
    deg.append(2 * 16 + 3)                  # the final task ends in a partial batch at n_edges
    return np.array(deg, dtype=np.int64)


def _task_facts(csr):
    """What the schedule holds, from its arrays (host mirror of the kernel's view of a task)."""
    rp = csr.rowptr.cpu().numpy().astype(np.int64)
    wr = csr.wave_row.cpu().numpy().astype(np.int64)
    ws = csr.wave_slot.cpu().numpy().astype(np.int64)
    lengths, cont_short, row_on_batch, empty_runs_in_task, split, most_rows = set(), set(), set(), 0, set(), 0
    for w in range(csr.n_waves):
        b, t = ws[w], ws[w + 1]
        lengths.add(int(t - b))
        r0, r1 = wr[w], wr[w + 1]
        if w > 0 and b < rp[r0]:
            split.add(int(r0) - 1)
            cont_short.add(int(min(rp[r0], t) - b))       # slots of the continued row in this task
        for r in range(r0, r1):
            if b < rp[r + 1] <= t:
                for U in (4, 8, 16):
                    if (rp[r + 1] - b) % U == 0:
                        row_on_batch.add(U)
        if r1 - r0 >= 64:                                   # the 64-row window refills inside the task
            empty_runs_in_task += 1
        most_rows = max(most_rows, int(r1 - r0))
    return {"lengths": lengths, "cont": cont_short, "row_on_batch": row_on_batch, "wide_tasks": empty_runs_in_task,
            "split": sorted(split), "most_rows": most_rows}


def _build(chunk, filler):
    _, _, CSR = _mods()
    deg = _degrees(chunk, filler=filler)
    N, E = len(deg), int(deg.sum())
    assert N <= 4096 and E <= 100_000, (N, E)
    g = torch.Generator().manual_seed(11)
    key = torch.repeat_interleave(torch.arange(N), torch.from_numpy(deg))
    other = torch.randint(N, (E,), generator=g)
    csr = CSR(key.to(DEV), other.to(DEV), N, N, chunk=chunk)
    return csr, key, other, _task_facts(csr)


@pytest.fixture(scope="module")
def graph():
    """(csr, key, other, facts): the engineered graph at chunk 64."""
    return _build(CHUNK, 400)


@pytest.fixture(scope="module")
def graph_wide():
    """The same construction at chunk 192: a task can hold more rows than two 64-row windows."""
    return _build(192, 100)


def test_schedule_holds_the_cases(graph):
    csr, _, _, facts = graph
    assert facts["lengths"] >= set(LENGTHS), sorted(facts["lengths"])
    assert facts["row_on_batch"] == {4, 8, 16}
    assert min(facts["cont"]) < 4, sorted(facts["cont"])            # a continuation shorter than every ring
    assert facts["wide_tasks"] >= 3                                  # 64 rows in one task: the row window refills
    assert csr.n_split == len(facts["split"]) > 3
    assert int(csr.wave_slot[-1]) == csr.n_edges and (csr.n_edges - int(csr.wave_slot[-2])) % 16 != 0


def _kernel_name(csr, x, w, reduce, bias, out):
    _lib, _, _ = _mods()
    lib = _lib.load()
    buf = ctypes.create_string_buffer(512)
    rc = lib.mp_aggregate_kernel_name(csr.struct("other"), _lib.ptr(w), x.data_ptr(), x.stride(0), x.shape[1],
                                      _lib.MP_REDUCE[reduce], _lib.ptr(bias), out.data_ptr(), out.stride(0), buf, 512,
                                      torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "mp_aggregate_kernel_name", lib)
    return buf.value.decode()


def _reference(x, key, other, w, bias, reduce, N):
    """(want, terms): the serial loop in slot order, then mean's division and the bias, each one fp32 operation."""
    want = S.gather_sum(x, other, key, w, N)
    terms = S.gather_sum(x.abs(), other, key, None if w is None else w.abs(), N)
    if reduce == "mean":
        cnt = torch.bincount(key, minlength=N).clamp(min=1).to(torch.float32).view(-1, 1)
        want, terms = want / cnt, terms / cnt
    if bias is not None:
        want, terms = want + bias, terms + bias.abs()
    return want, terms


def _check(csr, key, other, split, F, reduce, weighted, with_bias, far):
    _, ops, _ = _mods()
    N, E = csr.n_rows, csr.n_edges
    g = torch.Generator().manual_seed(F * 8 + weighted * 4 + with_bias * 2 + far)
    x = torch.randn(N, F, generator=g)
    w = torch.rand(E, generator=g) + 0.5 if weighted else None
    bias = torch.randn(F, generator=g) if with_bias else None
    xd = x.to(DEV)
    wd = csr.to_csr_order(w.to(DEV)) if weighted else None      # key is sorted: slot order is edge order
    bd = bias.to(DEV) if with_bias else None
    tune = {"flat_far_min_bytes": 1} if far else {}
    with _tuned(**tune):
        out, _ = ops._aggregate(csr, "other", xd, wd, reduce, 0, bd)
        again, _ = ops._aggregate(csr, "other", xd, wd, reduce, 0, bd)
        name = _kernel_name(csr, xd, wd, reduce, bd, out)
    torch.cuda.synchronize()
    # the scalar-batch flat kernel, the instance asked for: <Red, VEC, U, 64, false, true, ...>
    assert "k_agg_flat<" in name and ", 64, false, true" in name, name
    vec = 4 if F == 100 else 1
    batch = 8 if (far or vec == 4) else 16
    assert "%d, %d, 64, false, true" % (vec, batch) in name, name
    out, again = out.cpu(), again.cpu()
    assert torch.equal(out, again), "two runs on the same inputs differ"
    want, terms = _reference(x, key, other, w, bias, reduce, N)
    tol = 1e-5 * torch.clamp(terms, min=1.0)
    excess = ((out - want).abs() - tol).max().item()
    assert excess <= 0, "max excess %g" % excess
    whole = torch.ones(N, dtype=torch.bool)
    whole[split] = False
    assert torch.equal(out[whole], want[whole]), "rows summed by one task must be bit-exact"


@pytest.mark.parametrize("far", [0, 1])
@pytest.mark.parametrize("reduce,weighted,with_bias", [("sum", 1, 1), ("sum", 0, 0), ("mean", 1, 0), ("mean", 0, 1)])
@pytest.mark.parametrize("F", [64, 100, 128, 256])
def test_engineered_graph(graph, F, reduce, weighted, with_bias, far):
    csr, key, other, facts = graph
    _check(csr, key, other, facts["split"], F, reduce, weighted, with_bias, far)


def test_schedule_wide_tasks(graph_wide):
    csr, _, _, facts = graph_wide
    assert facts["most_rows"] > 128 and facts["lengths"] >= set(LENGTHS) and csr.n_split > 3


@pytest.mark.parametrize("F,reduce,weighted,with_bias,far", [(256, "sum", 1, 1, 1), (256, "sum", 1, 1, 0),
                                                             (100, "mean", 1, 0, 0), (64, "sum", 0, 1, 1)])
def test_wide_tasks(graph_wide, F, reduce, weighted, with_bias, far):
    """Runs of empty rows longer than two row windows inside one task."""
    csr, key, other, facts = graph_wide
    _check(csr, key, other, facts["split"], F, reduce, weighted, with_bias, far)


@pytest.mark.parametrize("F,reduce,with_bias", [(256, "sum", 1), (64, "mean", 0)])
def test_rows_start_from_out(graph, F, reduce, with_bias):
    """MP_FLAG_INIT_FROM_OUT: every owned row's accumulator starts from the value already in out.  On
    the ring instance that load is waited for where it is issued (begin_at<true>), on the near instance
    where it is first used; split hub rows and short continuations are in the graph.  The two
    instances must agree bit for bit, and both lie within the bound of init + sum."""
    _lib, ops, _ = _mods()
    csr, key, other, facts = graph
    assert len(facts["split"]) > 3 and min(facts["cont"]) < 4
    N, E = csr.n_rows, csr.n_edges
    g = torch.Generator().manual_seed(F + with_bias)
    x = torch.randn(N, F, generator=g)
    w = torch.rand(E, generator=g) + 0.5
    init = torch.randn(N, F, generator=g)
    bias = torch.randn(F, generator=g) if with_bias else None
    xd, wd = x.to(DEV), csr.to_csr_order(w.to(DEV))
    bd = bias.to(DEV) if with_bias else None
    got = {}
    for far in (0, 1):
        with _tuned(**({"flat_far_min_bytes": 1} if far else {})):
            out = init.to(DEV).clone()
            ops._aggregate(csr, "other", xd, wd, reduce, _lib.MP_FLAG_INIT_FROM_OUT, bd, out=out)
            name = _kernel_name(csr, xd, wd, reduce, bd, out)
        torch.cuda.synchronize()
        assert "1, %d, 64, false, true" % (8 if far else 16) in name, name
        got[far] = out.cpu()
    assert torch.equal(got[0], got[1]), "the ring instance and the near instance differ"
    # the row's sum starts at init and takes its terms in slot order; mean divides that whole sum
    want, terms = _reference(x, key, other, w, None, "sum", N)
    want, terms = init + want, init.abs() + terms
    if reduce == "mean":
        cnt = torch.bincount(key, minlength=N).clamp(min=1).to(torch.float32).view(-1, 1)
        want, terms = want / cnt, terms / cnt
    if bias is not None:
        want, terms = want + bias, terms + bias.abs()
    tol = 1e-5 * torch.clamp(terms, min=1.0)
    excess = ((got[1] - want).abs() - tol).max().item()
    assert excess <= 0, "max excess %g" % excess


@pytest.mark.parametrize("n_tasks", [1, 3, 4, 5, 31, 32, 33, 257])
def test_task_counts(n_tasks):
    """Grids of less than a block of waves, exactly a block, one wave more, and block counts that
    are and are not multiples of 8 (F = 256: 4 feature tiles, 2 blocks per tile and XCD pair)."""
    _, _, CSR = _mods()
    rng = np.random.RandomState(n_tasks)
    units = n_tasks * CHUNK - rng.randint(0, CHUNK - 1)
    deg = []
    while len(deg) + sum(deg) < units:
        deg.append(int(rng.choice([0, 1, 2, 5, 9, 17, 40, 130])))
    over = len(deg) + sum(deg) - units
    deg[-1] -= min(over, deg[-1])
    deg = np.array(deg, dtype=np.int64)
    N, E = len(deg), int(deg.sum())
    g = torch.Generator().manual_seed(n_tasks)
    key = torch.repeat_interleave(torch.arange(N), torch.from_numpy(deg))
    other = torch.randint(N, (E,), generator=g)
    csr = CSR(key.to(DEV), other.to(DEV), N, N, chunk=CHUNK)
    assert csr.n_waves == n_tasks, (csr.n_waves, n_tasks)
    split = _task_facts(csr)["split"]
    for far in (0, 1):
        _check(csr, key, other, split, 256, "sum", 1, 1, far)
