"""GatedGraphConv on the GPU against the float64 restatement tests/_ggc_ref.py: the fused GRU cell
(csrc/mp_gru.hip) forward and backward under the bound derived there, and the layer on the 257-node
graph of tests/test_gpu_arma.py (rebuilt here from the same seed and turned round, so that node 5
receives its 700 edges under this layer's flow; nodes 230.. isolated)."""
import copy
import functools
import math

import pytest
import torch

from tests import _ggc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_NODES = 257


def _nan(rows, cols, fill=None):
    """A NaN-filled device buffer (an unwritten element fails every comparison); fill: its first columns."""
    t = torch.full((rows, cols), float("nan"), device=DEV)
    if fill is not None:
        t[:, :fill.shape[1]] = fill.to(DEV)
    return t


def _within(got, ref, lim, what):
    err = (got.detach().cpu().double() - ref).abs()
    ratio = float((err / lim).max()) if err.numel() else 0.0
    print("%s: max |err| %.3g, max err / bound %.3g" % (what, float(err.max()) if err.numel() else 0.0, ratio))
    assert bool((err <= lim).all()), what
    return ratio


def check_cell(N, C, bias, what=""):
    """The cell forward (ops.gru_cell_forward) and backward (ops.gru_cell_backward) on N rows into NaN-filled
    outputs, the inputs' padding columns NaN, against R.cell / R.cell_backward; the padding columns of every
    output exactly zero; a second run bitwise equal.  Returns the largest err / bound."""
    from mi355_mp import ops
    g = torch.Generator().manual_seed(1000 * N + C)
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    P = ops.gru_width(C)
    a, h, dh = rnd(N, C), rnd(N, C), rnd(N, C)
    wc, wh = rnd(C, 3 * C) * 0.7 / math.sqrt(C), rnd(C, 3 * C) * 0.7 / math.sqrt(C)
    b_ih, b_hh = (rnd(3 * C) * 0.5, rnd(3 * C) * 0.5) if bias else (None, None)
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    # wh as the transposed view of a [3C, C] matrix (W_hh), the inputs' padding columns NaN
    pack = ops.gru_pack(dev(wc), dev(wh.t().contiguous()).t(), dev(b_ih), dev(b_hh), C)
    ad, hd = _nan(N, P, a), _nan(N, P, h)
    out, gates = ops.gru_cell_forward(ad, hd, pack, C, out=_nan(N, P), gates=_nan(N, 4 * P))
    ref, bound, _ = R.cell(a, h, wc, wh, b_ih, b_hh)
    worst = _within(out[:, :C], ref, bound, "%sh'" % what)
    assert float(out[:, C:].abs().sum()) == 0.0 and float(gates.view(N, 4, P)[:, :, C:].abs().sum()) == 0.0
    out2, gates2 = ops.gru_cell_forward(ad, hd, pack, C, want_gates=True)
    assert torch.equal(out, out2) and torch.equal(gates, gates2)
    assert torch.equal(ops.gru_cell_forward(ad, hd, pack, C)[0], out)          # inference: no gates stored
    dG, ddir = ops.gru_cell_backward(_nan(N, P, dh), hd, gates, C, dG=_nan(N, 4 * P), dh_dir=_nan(N, P))
    grads, dir_ref, scales = R.cell_backward(dh, h, [gates[:, k * P:k * P + C].cpu() for k in range(4)])
    for k, name in enumerate(("dn_pre", "dr_pre", "dz_pre", "dhn_pre")):
        worst = max(worst, _within(dG[:, k * P:k * P + C], grads[k], R.BOUND * scales[k] + 1e-30, what + name))
    worst = max(worst, _within(ddir[:, :C], dir_ref, R.BOUND * scales[4] + 1e-30, what + "dh_dir"))
    assert float(dG.view(N, 4, P)[:, :, C:].abs().sum()) == 0.0 and float(ddir[:, C:].abs().sum()) == 0.0
    dG2, ddir2 = ops.gru_cell_backward(_nan(N, P, dh), hd, gates, C)
    assert torch.equal(dG, dG2) and torch.equal(ddir, ddir2)
    return worst


# N: one row, an exact tile, a tile plus one row, three tiles and a tail; C: below one column block, padding inside
# a block, the full single slice, a partial second slice, the limit
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("C", [4, 20, 64, 80, 128])
@pytest.mark.parametrize("N", [1, 64, 65, 193])
def test_cell_forward_and_backward(N, C, bias):
    check_cell(N, C, bias)


@functools.lru_cache(maxsize=None)
def _graph():
    g = torch.Generator().manual_seed(1)
    row = torch.randint(0, 200, (2300,), generator=g)
    col = torch.randint(0, 230, (2300,), generator=g)
    ei = torch.stack([row, col])
    hub = torch.stack([torch.full((700,), 5, dtype=torch.int64), torch.randint(0, 230, (700,), generator=g)])
    ei = torch.cat([ei, ei[:, :40], hub], dim=1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)].flip(0).contiguous()
    assert int(torch.bincount(ei[1], minlength=N_NODES)[5]) >= 700 and int(ei.max()) < 230
    return ei, torch.rand(ei.shape[1], generator=g) + 0.5


def _grads(out, gout, params):
    return [out.detach()] + list(torch.autograd.grad((out * gout).sum(), params))


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("aggr", ["add", "mean"])
def test_layer_matches_the_reference(aggr, weighted):
    """C = 40 (P = 48), L = 3, a 9-wide input.  Tolerance, per tensor (the output and each parameter's gradient):
    4 x the max-norm error of the layer's own recipe() run in fp32 torch CPU ops against the same fp64
    reference; the 4 covers the other summation orders (MFMA k order and slot-order aggregation against
    BLAS and index_add_)."""
    from torch_geometric.nn import GatedGraphConv
    C, L, Fin = 40, 3, 9
    ei, ew = _graph()
    ew = ew if weighted else None
    torch.manual_seed(3)
    cpu = GatedGraphConv(C, L, aggr=aggr)
    x, gout = torch.randn(N_NODES, Fin), torch.randn(N_NODES, C)
    names = [n for n, _ in cpu.named_parameters()]
    p64 = [p.detach().double().requires_grad_(True) for p in cpu.parameters()]
    rnn = {n[4:]: p for n, p in zip(names, p64) if n.startswith("rnn.")}
    ref = _grads(R.layer(x, ei, ew, p64[names.index("weight")], rnn, aggr), gout.double(), p64)
    rec = _grads(cpu.recipe(x, ei, ew), gout, list(cpu.parameters()))
    gpu = copy.deepcopy(cpu).to(DEV)
    xd, eid, ewd = x.to(DEV), ei.to(DEV), None if ew is None else ew.to(DEV)
    assert gpu.fused(xd, ewd)
    out = gpu(xd, eid, ewd)
    got = _grads(out, gout.to(DEV), list(gpu.parameters()))
    assert torch.equal(gpu(xd, eid, ewd, form="fused"), out)
    for name, g_, r_, c_ in zip(["out"] + names, got, ref, rec):
        tol = 4 * float((c_.double() - r_).abs().max())
        err = float((g_.cpu().double() - r_).abs().max())
        print("%s: |fused - ref| %.3g, 4 x |recipe fp32 - ref| %.3g" % (name, err, tol))
        assert err <= tol, name


@pytest.mark.parametrize("C,aggr", [(132, "add"), (16, "max")])
def test_outside_the_fused_path_takes_the_recipe(C, aggr):
    from torch_geometric.nn import GatedGraphConv
    ei, ew = _graph()
    torch.manual_seed(4)
    layer = GatedGraphConv(C, 2, aggr=aggr).to(DEV)
    x, eid, ewd = torch.randn(N_NODES, 7, device=DEV), ei.to(DEV), ew.to(DEV)
    assert not layer.fused(x, ewd)
    assert torch.allclose(layer(x, eid, ewd), layer.recipe(x, eid, ewd), atol=1e-5)
    with pytest.raises(ValueError):
        layer(x, eid, ewd, form="fused")
