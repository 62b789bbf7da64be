"""The attention readout (csrc/mp_glob.hip) and the two layers on it, Set2Set
and GlobalAttention, on the GPU against the float64 restatement
tests/_glob_ref.py.

Bound, every float comparison: |got - want| <= 1e-4 * max(1, |want|) entrywise
against float64 (the project's bound for softmax layers; the upstream recipe in
fp32 keeps a margin of 3x or more to it at this input scale: randn x, q, dr).
Graph sizes follow ops.readout_path / ops.readout_chunk: t - 1, t, t + 1 around
both path boundaries, k * chunk - 1, k * chunk, k * chunk + 1 for k = 1, 2, 5,
and the fixed small set with its graph without nodes.  Each parity test prints
its worst |err| / max(1, |want|) per tensor.
"""
import pytest
import torch

from tests import _glob_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 1e-4
FIXED = [1, 0, 2, 18, 63, 64, 65, 9, 29]
WIDTHS = [1, 3, 4, 33, 64, 65, 200, 260]


def _ops():
    from mi355_mp import ops
    return ops


def boundaries(C):
    """(t1, t2, chunk): the first n_g on path 1, the first on path 2, the chunk."""
    ops = _ops()
    t = []
    for want in (1, 2):
        lo, hi = 0, 1 << 24                       # path(lo) < want <= path(hi); the path is monotone in n_g
        assert ops.readout_path(hi, C) == 2
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if ops.readout_path(mid, C) >= want else (mid, hi)
        t.append(hi)
    return t[0], t[1], ops.readout_chunk(C)


def sizes_for(C):
    t1, t2, chunk = boundaries(C)
    s = list(FIXED) + [t1 - 1, t1, t1 + 1, t2 - 1, t2, t2 + 1]
    for k in (1, 2, 5):
        s += [k * chunk - 1, k * chunk, k * chunk + 1]
    ops = _ops()
    assert {ops.readout_path(n, C) for n in s} == {0, 1, 2} and ops.readout_path(5 * chunk - 1, C) == 2
    return s + [0]                                # a trailing graph without nodes


def layout_of(sizes):
    ops = _ops()
    starts = torch.tensor([0] + list(torch.tensor(sizes).cumsum(0)), dtype=torch.int64)
    return ops.BatchLayout(starts.to(DEV), len(sizes), max(sizes) if sizes else 0, 0, int(starts[-1])), starts


def worst(got, want):
    want = want.double()
    return float(((got.detach().cpu().double() - want).abs() / want.abs().clamp(min=1)).max()) if want.numel() else 0.0


def check(report, name, got, want):
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), "%s has entries that are not finite (unwritten?)" % name
    w = worst(got, want)
    report[name] = max(report.get(name, 0.0), w)
    assert w <= BOUND, "%s: worst |err| / max(1, |want|) = %.3g" % (name, w)


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def raw_forward(x, layout, q=None, score=None, pad=3, q_copy=False, want_alpha=True):
    """mp_attention_readout_f32 on NaN-filled outputs: out [G, 2C + pad] written
    at column C, x strided as given.  Returns (buf, e, stats, alpha)."""
    from mi355_mp import _lib
    ops = _ops()
    nat = _lib.native()
    n, C = x.shape
    G = layout.n_graphs
    buf, e, stats, alpha = nan(G, 2 * C + pad), nan(n), nan(G, 2), nan(n)
    r = buf[:, C:2 * C]
    qo = buf[:, :C] if q_copy else None
    wsb = nat.mp_readout_workspace(n, G, layout.max_n, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    ops._count_call(nat, "mp_attention_readout_f32", x.data_ptr(), x.stride(0), n, C, layout.starts.data_ptr(), G,
                    layout.max_n, _lib.ptr(q), 0 if q is None else q.stride(0), _lib.ptr(score), r.data_ptr(),
                    buf.stride(0), ops._strided_bytes(r), _lib.ptr(qo), 0 if qo is None else ops._strided_bytes(qo),
                    e.data_ptr(), _lib.nbytes(e), stats.data_ptr(), _lib.nbytes(stats),
                    alpha.data_ptr() if want_alpha else None, _lib.nbytes(alpha) if want_alpha else 0, ws.data_ptr(),
                    wsb, _lib.stream_ptr(torch.device(DEV)))
    return buf, e, stats, alpha


def raw_backward(dr, x, layout, e, stats, r, q=None, pad=2):
    """mp_attention_readout_bwd_f32 on NaN-filled outputs (dx strided C + pad)."""
    from mi355_mp import _lib
    ops = _ops()
    nat = _lib.native()
    n, C = x.shape
    G = layout.n_graphs
    dxb = nan(n, C + pad)
    dx = dxb[:, :C]
    dq = nan(G, C) if q is not None else None
    ds = nan(n) if q is None else None
    wsb = nat.mp_readout_workspace(n, G, layout.max_n, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    ops._count_call(nat, "mp_attention_readout_bwd_f32", dr.data_ptr(), dr.stride(0), x.data_ptr(), x.stride(0), n, C,
                    layout.starts.data_ptr(), G, layout.max_n, _lib.ptr(q), 0 if q is None else q.stride(0),
                    e.data_ptr(), stats.data_ptr(), r.data_ptr(), r.stride(0), dx.data_ptr(), dxb.stride(0),
                    ops._strided_bytes(dx), _lib.ptr(dq), C, _lib.nbytes(dq), _lib.ptr(ds), _lib.nbytes(ds),
                    ws.data_ptr(), wsb, _lib.stream_ptr(torch.device(DEV)))
    return dxb, dq, ds


def draw(sizes, C, seed, ldx=None):
    g = torch.Generator().manual_seed(seed)
    n, G = sum(sizes), len(sizes)
    ldx = C + 5 if ldx is None else ldx
    xw = torch.randn(n, ldx, generator=g)
    return xw, torch.randn(G, C, generator=g), torch.randn(n, generator=g), torch.randn(G, C, generator=g)


# 1. the kernels against the checker -------------------------------------------------

@pytest.mark.parametrize("mode", ["query", "score"])
@pytest.mark.parametrize("C", WIDTHS)
def test_kernels_against_float64(C, mode):
    sizes = sizes_for(C)
    layout, starts = layout_of(sizes)
    xw, q, score, dr = draw(sizes, C, 100 + C)
    x = xw[:, :C]
    kw = {"q": q} if mode == "query" else {"score": score}
    want_r, want_e, want_m, want_den, want_a = R.readout(x, starts, **kw)
    grads = R.readout_grads(x, starts, dr, **kw)
    xd = xw.to(DEV)[:, :C]                                           # ldx = C + 5: scalar loads at every C
    dkw = {k: v.to(DEV) for k, v in kw.items()}
    report = {}
    buf, e, stats, alpha = raw_forward(xd, layout, q_copy=mode == "query", **dkw)
    check(report, "r", buf[:, C:2 * C], want_r)
    check(report, "e", e, want_e)
    check(report, "m", stats[:, 0], want_m)
    check(report, "den", stats[:, 1], want_den)
    check(report, "alpha", alpha, want_a)
    assert bool(torch.isnan(buf[:, 2 * C:]).all()), "padding beyond the written columns was touched"
    if mode == "query":
        assert torch.equal(buf[:, :C].cpu(), q), "q was not copied into columns 0 .. C"
    else:
        assert bool(torch.isnan(buf[:, :C]).all()), "the other half of the buffer was touched"
    empty = [i for i, s in enumerate(sizes) if s == 0]
    assert float(buf[empty, C:2 * C].abs().max()) == 0.0 and float(stats[empty].abs().max()) == 0.0
    drd = dr.to(DEV)
    dxb, dq, ds = raw_backward(drd, xd, layout, e, stats, buf[:, C:2 * C], q=dkw.get("q"))
    check(report, "dx", dxb[:, :C], grads["dx"])
    assert bool(torch.isnan(dxb[:, C:]).all())
    if mode == "query":
        check(report, "dq", dq, grads["dq"])
        assert float(dq[empty].abs().max()) == 0.0
    else:
        check(report, "dscore", ds, grads["dscore"])
    print("C=%d %s worst |err|/max(1,|want|): %s" % (C, mode, {k: "%.2g" % v for k, v in report.items()}))


@pytest.mark.parametrize("C", [4, 64, 260, 1028])
def test_sixteen_byte_path_and_autograd(C):
    """Contiguous rows (the 16-byte loads; C = 1028: two channel tiles of them)
    through ops.attention_readout and torch's autograd, both modes; gradients
    nobody asks for are not computed."""
    ops = _ops()
    sizes = sizes_for(C)
    layout, starts = layout_of(sizes)
    xw, q, score, dr = draw(sizes, C, 200 + C, ldx=C)
    report = {}
    for kw in ({"q": q}, {"score": score}):
        want = R.readout(xw, starts, **kw)[0]
        grads = R.readout_grads(xw, starts, dr, **kw)
        xd = xw.to(DEV).requires_grad_(True)
        dkw = {k: v.to(DEV).requires_grad_(True) for k, v in kw.items()}
        r = ops.attention_readout(xd, layout, **dkw)
        check(report, "r", r, want)
        (r * dr.to(DEV)).sum().backward()
        check(report, "dx", xd.grad, grads["dx"])
        for k, v in dkw.items():
            check(report, "d" + k, v.grad, grads["d" + k])
        # only x needs a gradient
        xd2 = xw.to(DEV).requires_grad_(True)
        r2 = ops.attention_readout(xd2, layout, **{k: v.detach() for k, v in dkw.items()})
        (r2 * dr.to(DEV)).sum().backward()
        assert torch.equal(xd2.grad, xd.grad) and torch.equal(r2, r)
    print("C=%d contiguous worst: %s" % (C, {k: "%.2g" % v for k, v in report.items()}))
    with pytest.raises(RuntimeError):
        ops.attention_readout(xw, layout, q=q.to(DEV))               # a host tensor


@pytest.mark.parametrize("form", ["query", "score", "query_out"])
def test_backward_of_a_reduction_over_graphs(form):
    """out.sum(0) hands backward a broadcast gradient (row stride 0): both
    modes, and the out= / col= form whose q columns carry gradient too."""
    ops = _ops()
    C = 8
    sizes = [3, 0, 70, 150, 1100, 1]                                  # every path, a graph without nodes
    assert {ops.readout_path(n, C) for n in sizes} == {0, 1, 2}
    layout, starts = layout_of(sizes)
    xw, q, score, _ = draw(sizes, C, 400, ldx=C)
    G = len(sizes)
    xr = xw.double().requires_grad_(True)
    qr, sr = q.double().requires_grad_(True), score.double().requires_grad_(True)
    xd = xw.to(DEV).requires_grad_(True)
    qd, sd = q.to(DEV).requires_grad_(True), score.to(DEV).requires_grad_(True)
    rep = {}
    if form == "score":
        want = R.readout(xr, starts, score=sr)[0]
        out = ops.attention_readout(xd, layout, score=sd)
    elif form == "query":
        want = R.readout(xr, starts, q=qr)[0]
        out = ops.attention_readout(xd, layout, q=qd)
    else:
        want = torch.cat([qr, R.readout(xr, starts, q=qr)[0]], dim=-1)
        out = ops.attention_readout(xd, layout, q=qd, out=torch.full((G, 2 * C), float("nan"), device=DEV), col=C)
    check(rep, "out", out, want.detach())
    want.sum(0).square().sum().backward()
    out.sum(0).square().sum().backward()
    check(rep, "dx", xd.grad, xr.grad)
    if form == "score":
        check(rep, "dscore", sd.grad, sr.grad)
    else:
        check(rep, "dq", qd.grad, qr.grad)
    # and a mean over graphs of a layer's output
    from torch_geometric.nn import Set2Set
    torch.manual_seed(3)
    layer = Set2Set(C, 2).to(DEV)
    batch = _batch(sizes)
    ref = R.lstm64(layer.lstm)
    xr2 = xw.double().requires_grad_(True)
    R.set2set(xr2, batch, ref, 2).mean(0).square().sum().backward()
    xd2 = xw.to(DEV).requires_grad_(True)
    layer(xd2, batch.to(DEV)).mean(0).square().sum().backward()
    check(rep, "Set2Set dx", xd2.grad, xr2.grad)
    with pytest.raises(ValueError):
        ops.attention_readout(xd, layout, q=qd, out=torch.zeros((G, 2 * C), device=DEV, requires_grad=True), col=C)


# 2. stability ---------------------------------------------------------------------------

def test_large_scores_need_the_max_subtracted():
    C = 64
    sizes = sizes_for(C)
    layout, starts = layout_of(sizes)
    xw, q, score, dr = draw(sizes, C, 7, ldx=C)
    score = 90 + 20 * torch.rand(sum(sizes), generator=torch.Generator().manual_seed(8))   # exp(90) overflows fp32
    buf, e, stats, _ = raw_forward(xw.to(DEV), layout, score=score.to(DEV))
    rep = {}
    check(rep, "r", buf[:, C:2 * C], R.readout(xw, starts, score=score)[0])
    dxb, _, ds = raw_backward(dr.to(DEV), xw.to(DEV), layout, e, stats, buf[:, C:2 * C])
    g = R.readout_grads(xw, starts, dr, score=score)
    check(rep, "dx", dxb[:, :C], g["dx"])
    check(rep, "dscore", ds, g["dscore"])
    q4 = 4 * q                                                        # |e| up to about 130
    buf, e, stats, _ = raw_forward(xw.to(DEV), layout, q=q4.to(DEV))
    want = R.readout(xw, starts, q=q4)
    assert float(want[1].abs().max()) > 80
    check(rep, "r(4q)", buf[:, C:2 * C], want[0])
    dxb, dq, _ = raw_backward(dr.to(DEV), xw.to(DEV), layout, e, stats, buf[:, C:2 * C], q=q4.to(DEV))
    g = R.readout_grads(xw, starts, dr, q=q4)
    check(rep, "dx(4q)", dxb[:, :C], g["dx"])
    check(rep, "dq(4q)", dq, g["dq"])
    print("stability worst: %s" % {k: "%.2g" % v for k, v in rep.items()})


def test_shift_invariance():
    C = 33
    sizes = sizes_for(C)
    layout, starts = layout_of(sizes)
    xw, _, score, _ = draw(sizes, C, 9, ldx=C)
    a = raw_forward(xw.to(DEV), layout, score=score.to(DEV))[0][:, C:2 * C]
    b = raw_forward(xw.to(DEV), layout, score=(score + 100).to(DEV))[0][:, C:2 * C]
    # score + 100 rounds each score to a multiple of 2^-17 or so: compare both to the float64 value of their own input
    rep = {}
    check(rep, "r", a, R.readout(xw, starts, score=score)[0])
    check(rep, "r(+100)", b, R.readout(xw, starts, score=score + 100)[0])
    check(rep, "r vs r(+100)", b, R.readout(xw, starts, score=score)[0])


# 3. bitwise -----------------------------------------------------------------------------

@pytest.mark.parametrize("C", [33, 64])
def test_bits_repeat_and_do_not_depend_on_the_batch(C):
    t1, t2, chunk = boundaries(C)
    sizes = [t1 - 1, 0, t1 + 3, t2 + chunk + 1, 5, t2 - 1]          # paths 0, -, 1, 2, 0, 1
    layout, starts = layout_of(sizes)
    xw, q, score, dr = draw(sizes, C, 300 + C, ldx=C + (4 if C % 4 == 0 else 1))
    xd, qd, drd = xw.to(DEV)[:, :C], q.to(DEV), dr.to(DEV)
    pad = 4 if C % 4 == 0 else 3                                      # C = 64: every stride allows the 16-byte form
    runs = []
    for _ in range(2):
        buf, e, stats, _ = raw_forward(xd, layout, q=qd, pad=pad)
        dxb, dq, _ = raw_backward(drd, xd, layout, e, stats, buf[:, C:2 * C], q=qd, pad=pad)
        runs.append((buf[:, C:2 * C].clone(), stats, dxb[:, :C].clone(), dq))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs of one call differ"
    r, stats, dx, dq = runs[0]
    for g, n_g in enumerate(sizes):
        if n_g == 0:
            continue
        b, t = int(starts[g]), int(starts[g + 1])
        one, _ = layout_of([n_g])
        x1 = xd[b:t]                                                  # whole rows: strides and alignment class kept
        buf1, e1, s1, _ = raw_forward(x1, one, q=qd[g:g + 1], pad=pad)
        dxb1, dq1, _ = raw_backward(drd[g:g + 1], x1, one, e1, s1, buf1[:, C:2 * C], q=qd[g:g + 1], pad=pad)
        assert torch.equal(buf1[:, C:2 * C], r[g:g + 1]), ("r", g, n_g)
        assert torch.equal(s1, stats[g:g + 1]), ("stats", g, n_g)
        assert torch.equal(dxb1[:, :C], dx[b:t]), ("dx", g, n_g)
        assert torch.equal(dq1, dq[g:g + 1]), ("dq", g, n_g)


# 4. the layers --------------------------------------------------------------------------

def _batch(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


LAYER_SIZES = [1, 2, 18, 0, 63, 64, 65, 9, 29, 150, 1100]           # graph 3 has no node; C = 8: paths 0, 1, 2


@pytest.mark.parametrize("steps,num_layers", [(3, 1), (2, 2)])
def test_set2set_against_float64(steps, num_layers):
    from torch_geometric.nn import Set2Set
    C = 8
    ops = _ops()
    assert {ops.readout_path(n, C) for n in LAYER_SIZES} == {0, 1, 2}
    torch.manual_seed(5)
    layer = Set2Set(C, steps, num_layers).to(DEV)
    batch = _batch(LAYER_SIZES)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(batch.numel(), C, generator=g)
    w = torch.randn(len(LAYER_SIZES), 2 * C, generator=g)
    ref = R.lstm64(layer.lstm)
    xr = x.double().requires_grad_(True)
    want = R.set2set(xr, batch, ref, steps)
    (want * w.double()).sum().backward()
    rep = {}
    xd = x.to(DEV).requires_grad_(True)
    out = layer(xd, batch.to(DEV))
    check(rep, "out", out, want.detach())
    (out * w.to(DEV)).sum().backward()
    check(rep, "dx", xd.grad, xr.grad)
    for (name, p), (_, pr) in zip(layer.lstm.named_parameters(), ref.named_parameters()):
        check(rep, name, p.grad, pr.grad)
    # the recipe path on the same input: a shuffled (unsorted) batch is the same set function
    perm = torch.randperm(batch.numel(), generator=g)
    assert ops.cached_batch_layout(batch[perm].to(DEV), batch.numel()).unsorted > 0
    layer.zero_grad()
    xs = x[perm].to(DEV).requires_grad_(True)
    out_s = layer(xs, batch[perm].to(DEV))
    check(rep, "out(unsorted)", out_s, want.detach())
    check(rep, "fused vs recipe", out, out_s.detach().cpu())
    (out_s * w.to(DEV)).sum().backward()
    check(rep, "dx(unsorted)", xs.grad, xr.grad[perm])
    print("Set2Set(%d, %d, %d) worst: %s" % (C, steps, num_layers, {k: "%.2g" % v for k, v in rep.items()}))


@pytest.mark.parametrize("with_nn", [False, True])
def test_global_attention_against_float64(with_nn):
    from torch_geometric.nn import GlobalAttention
    C, Co = 8, 5
    torch.manual_seed(11)
    gate = torch.nn.Sequential(torch.nn.Linear(C, 6), torch.nn.ReLU(), torch.nn.Linear(6, 1))
    nn = torch.nn.Linear(C, Co) if with_nn else None
    layer = GlobalAttention(gate, nn).to(DEV)
    import copy
    gate64 = copy.deepcopy(gate).cpu().double()
    nn64 = copy.deepcopy(nn).cpu().double() if with_nn else None
    sizes = [s for s in LAYER_SIZES if s]                             # batch[-1] + 1 graphs, then two more through size
    batch = _batch(sizes)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(batch.numel(), C, generator=g)
    rep = {}
    for size in (None, len(sizes) + 2):
        G = len(sizes) if size is None else size
        w = torch.randn(G, Co if with_nn else C, generator=g)
        xr = x.double().requires_grad_(True)
        want = R.global_attention(xr, batch, size, gate64, nn64)
        (want * w.double()).sum().backward()
        xd = x.to(DEV).requires_grad_(True)
        out = layer(xd, batch.to(DEV), size)
        check(rep, "out", out, want.detach())
        layer.zero_grad()
        (out * w.to(DEV)).sum().backward()
        check(rep, "dx", xd.grad, xr.grad)
        want_g = torch.autograd.grad((R.global_attention(x.double(), batch, size, gate64, nn64) * w.double()).sum(),
                                     list(gate64.parameters()) + (list(nn64.parameters()) if with_nn else []))
        n_gate = len(list(gate64.parameters()))
        for p, pw in zip(gate.parameters(), want_g[:n_gate]):
            check(rep, "d gate_nn", p.grad, pw)
        if with_nn:                                                   # nn's parameters are what dx feeds here
            assert len(want_g) == n_gate + 2
            for p, pw in zip(nn.parameters(), want_g[n_gate:]):
                check(rep, "d nn", p.grad, pw)
        if size is not None:
            assert float(out.detach()[len(sizes):].abs().max()) == 0.0
        # unsorted: the recipe path
        perm = torch.randperm(batch.numel(), generator=g)
        perm = torch.cat([perm[perm != batch.numel() - 1], torch.tensor([batch.numel() - 1])])   # batch[-1] stays the max
        out_s = layer(x[perm].to(DEV), batch[perm].to(DEV), size)
        check(rep, "out(unsorted)", out_s, want.detach())
        check(rep, "fused vs recipe", out, out_s.detach().cpu())
    # the layout for a size beyond the batch's graphs is built once per batch tensor and size
    from torch_geometric.nn.glob._readout import fused_layout
    bd, xd = batch.to(DEV), x.to(DEV)
    ext = fused_layout(xd, bd, len(sizes) + 2)
    assert ext is fused_layout(xd, bd, len(sizes) + 2) and ext.n_graphs == len(sizes) + 2
    assert fused_layout(xd, bd, len(sizes)).n_graphs == len(sizes) and fused_layout(xd, bd, len(sizes) - 1) is None
    print("GlobalAttention(nn=%s) worst: %s" % (with_nn, {k: "%.2g" % v for k, v in rep.items()}))


def test_one_dimensional_x_and_no_batch():
    from torch_geometric.nn import GlobalAttention, Set2Set
    torch.manual_seed(13)
    g = torch.Generator().manual_seed(14)
    gate = torch.nn.Linear(1, 1)
    layer = GlobalAttention(gate).to(DEV)
    sizes = [3, 70, 1, 200]
    batch = _batch(sizes)
    x = torch.randn(batch.numel(), generator=g)
    import copy
    want = R.global_attention(x, batch, None, copy.deepcopy(gate).cpu().double())
    rep = {}
    check(rep, "1-D x", layer(x.to(DEV), batch.to(DEV)), want.detach())
    # batch = None is the one-graph batch
    x2 = torch.randn(1500, 4, generator=g).to(DEV)
    zeros = torch.zeros(1500, dtype=torch.int64, device=DEV)
    gate4 = torch.nn.Linear(4, 1).to(DEV)
    ga = GlobalAttention(gate4)
    assert torch.equal(ga(x2, None), ga(x2, zeros))
    s2s = Set2Set(4, 2).to(DEV)
    assert torch.equal(s2s(x2, None), s2s(x2, zeros))
    check(rep, "Set2Set one graph", s2s(x2, zeros), R.set2set(x2.cpu(), zeros.cpu(), R.lstm64(s2s.lstm), 2).detach())


# 5. edge cases --------------------------------------------------------------------------

def test_no_nodes_one_graph_single_nodes():
    ops = _ops()
    C = 5
    # N = 0: no graphs at all, and graphs that are all empty
    for sizes in ([], [0, 0, 0]):
        layout, _ = layout_of(sizes)
        x = torch.zeros((0, C), device=DEV, requires_grad=True)
        q = torch.randn(len(sizes), C, device=DEV, requires_grad=True)
        r = ops.attention_readout(x, layout, q=q)
        assert r.shape == (len(sizes), C) and float(r.detach().abs().sum()) == 0.0
        if sizes:
            r.sum().backward()
            assert x.grad.shape == (0, C) and float(q.grad.abs().sum()) == 0.0
        r = ops.attention_readout(x.detach(), layout, score=torch.zeros(0, device=DEV))
        assert r.shape == (len(sizes), C) and float(r.abs().sum()) == 0.0
    # G = 1
    g = torch.Generator().manual_seed(15)
    x, q = torch.randn(77, C, generator=g), torch.randn(1, C, generator=g)
    layout, starts = layout_of([77])
    rep = {}
    check(rep, "G = 1", ops.attention_readout(x.to(DEV), layout, q=q.to(DEV)), R.readout(x, starts, q=q)[0])
    # one node per graph: a = 1 and r = x exactly
    x = torch.randn(300, C, generator=g)
    layout, _ = layout_of([1] * 300)
    buf, e, stats, alpha = raw_forward(x.to(DEV), layout, q=torch.randn(300, C, generator=g).to(DEV))
    assert torch.equal(buf[:, C:2 * C].cpu(), x) and torch.equal(alpha.cpu(), torch.ones(300))
    assert torch.equal(stats[:, 1].cpu(), torch.ones(300)) and torch.equal(stats[:, 0], e)
    r = ops.attention_readout(x.to(DEV), layout, score=torch.randn(300, generator=g).to(DEV))
    assert torch.equal(r.cpu(), x)
