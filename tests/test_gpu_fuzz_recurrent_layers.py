"""Layer-level fuzzing of ARMAConv and GatedGraphConv, the sibling of test_gpu_fuzz_conv_layers.py for the
recurrent layers, with the input-view and empty-graph checks of ARMAConv, GatedGraphConv, AGNNConv and
DNAConv.

The inputs come from tests/_fuzz_cases.py (shared with the CPU test tests/test_recurrent_cases_host.py, which
runs every pinned example through the restatements alone); the references are the float64 restatements
tests/_arma_ref.py and tests/_ggc_ref.py.  Every draw is valid by construction (no assume, no skip).

ARMAConv: the output and the gradients of x, ws, vs and bias within |err| <= 1e-5 * sum |terms|, the ReLU
masks of the backward taken from the GPU's hidden states as test_gpu_arma._gpu_masks takes them (its cap --
at most 0.5 % of a draw's pre-activations within the bound of zero -- is a condition of the test).
GatedGraphConv: values within 1e-5 * max(1, |ref|) + 4 * own, gradients within 1e-4 * max(1, |ref|) + 4 * own,
own = the max-norm error of the layer's recipe in fp32 on the CPU against the same float64 reference (the
bound tests/test_gpu_fuzz_layers.py uses for ill-conditioned layers).
"""
import copy

import pytest
import torch
import torch.nn.functional as F
from hypothesis import example, given, settings, strategies as st

from tests import _arma_ref as AR, _fuzz_cases as Z, _ggc_ref as GR, _recurrent_lane_cases as K
from tests import test_gpu_arma as TA
from tests.test_gpu_fuzz_conv_layers import _pinned, _x_view
from tests.test_gpu_fuzz_layers import _N_EX, _SETTINGS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_COSTLY = dict(_SETTINGS, max_examples=max(10, _N_EX // 2))
_COSTLIEST = dict(_SETTINGS, max_examples=max(10, _N_EX // 3))


# --------------------------------------------------------------------------
# a. ARMAConv
# --------------------------------------------------------------------------

def _arma_layer(p, ws, vs, bias, act):
    from torch_geometric.nn import ARMAConv
    (k, c) = p["kc"]
    layer = ARMAConv(p["F_in"], c, k, p["T"], shared_weights=p["shared"], act=act, bias=p["bias"])
    with torch.no_grad():
        for dst, src in zip(list(layer.ws) + list(layer.vs) + (list(layer.bias) if p["bias"] else []),
                            ws + vs + (bias or [])):
            assert dst.shape == src.shape
            dst.copy_(src)
    return layer.to(DEV)


def _stack(h):
    """A recorded [K, N, C] state in the kernels' stacked [N, K * C] layout (no padding columns)."""
    return h.permute(1, 0, 2).reshape(h.shape[1], -1)


@settings(**_COSTLY)
@given(N=st.integers(1, 150), deg=st.floats(0.0, 8.0), loops=st.sampled_from([0.0, 0.2, 1.0]),
       F_in=st.integers(1, 20), kc=st.sampled_from(K.ARMA_CASES + (K.ARMA_OUTSIDE,)), T=st.integers(1, 3),
       shared=st.booleans(), act=st.sampled_from(["relu", None]), bias=st.booleans(), weighted=st.booleans(),
       form=st.sampled_from([None, "fused"]), seed=st.integers(0, 1 << 16))
@_pinned(Z.ARMA_PINNED)
def test_fuzz_armaconv_layer(N, deg, loops, F_in, kc, T, shared, act, bias, weighted, form, seed):
    """ARMAConv(F_in, C, K, T, shared_weights, act, bias)(x, edge_index, edge_weight, form): the output and the
    gradients of x and of every parameter against the float64 restatement.  A (K, C) outside arma_ok takes
    the recipe (and refuses form="fused"); its ReLU masks are recorded from the recipe's own activations.
    Pinned (Z.ARMA_PINNED): N = 1 without edges and with self loops only, N = 5 without edges, every edge a
    loop, deg 0.3, one example per task width L, T = 3 with K = 1, C = 1, the pair outside arma_ok."""
    from mi355_mp import ops
    from mi355_mp.graph import graph_for
    p = dict(N=N, deg=deg, loops=loops, F_in=F_in, kc=kc, T=T, shared=shared, act=act, bias=bias, weighted=weighted,
             form=form, seed=seed)
    ei, ew, x, ws, vs, bs, gout = Z.arma_inputs(p)
    k, c = kc
    inside = ops.arma_ok(k, c)
    assert inside == K.arma_ok(k, c)
    what = "N=%d E=%d F=%d K=%d C=%d T=%d %s %s form=%s" % (N, ei.shape[1], F_in, k, c, T, "shared" if shared else "",
                                                          act, form)
    recorded = []

    def recording_relu(t):                                            # (not F.relu: the layer takes the recipe)
        recorded.append(t.clamp(min=0))
        return recorded[-1]

    layer = _arma_layer(p, ws, vs, bs, (F.relu if inside else recording_relu) if act == "relu" else None)
    xd, eid, ewd = x.to(DEV).requires_grad_(True), ei.to(DEV), None if ew is None else ew.to(DEV)
    assert layer.fused(xd, ewd) == inside, what
    if not inside and form == "fused":
        with pytest.raises(ValueError):
            layer(xd, eid, ewd, form="fused")
        form = None
    out = layer(xd, eid, ewd, form=form)
    assert tuple(out.shape) == (N, c), what
    out.backward(gout.to(DEV))
    args = (x, ei, ew, ws, vs, bs, T, shared)
    r_out, _, r_pre = AR.forward(*args, act)
    a_out, _, a_pre = AR.forward(*args, act, absolute=True)
    worst = AR.assert_bound(out, r_out, a_out, "out " + what)
    masks = None
    if act == "relu":
        if inside:
            graph = graph_for(eid, N, N, "target_to_source")
            Hs = ops.arma_propagate(graph, xd.detach(), list(layer.ws), list(layer.vs),
                                    list(layer.bias) if bias else None, k, c, T, shared, True, 0.0, False,
                                    want_hidden=True, edge_weight=ewd)[1]
        else:
            Hs = [_stack(h.detach()) for h in recorded]
        assert len(Hs) == T
        masks = TA._gpu_masks(Hs, r_pre, a_pre, k, c)
    ref = AR.gradients(*args, gout, act=act, masks=masks)
    absv = AR.gradients(*args, gout, act=act, masks=masks, absolute=True)
    worst = max(worst, AR.assert_bound(xd.grad, ref[0], absv[0], "d x " + what))
    for name, params, i in (("ws", layer.ws, 1), ("vs", layer.vs, 2), ("bias", layer.bias if bias else [], 3)):
        for j, q in enumerate(params):
            worst = max(worst, AR.assert_bound(q.grad, ref[i][j], absv[i][j], "d %s[%d] %s" % (name, j, what)))
    print("ARMAConv %s: L = %s, max err / bound %.3g" % (what, K.arma_lanes(k, c) if inside else "recipe",
                                                         worst / AR.BOUND))


# --------------------------------------------------------------------------
# b. GatedGraphConv
# --------------------------------------------------------------------------

def _grads(out, gout, leaves):
    return [out.detach()] + list(torch.autograd.grad((out * gout).sum(), leaves))


@settings(**_COSTLY)
@given(N=st.integers(1, 150), deg=st.floats(0.0, 8.0), loops=st.sampled_from([0.0, 0.2, 1.0]),
       C=st.sampled_from([1, 5, 16, 40, 90, 100, 128]), L=st.integers(1, 3), xcols=st.integers(0, 128),
       aggr=st.sampled_from(["add", "mean"]), bias=st.booleans(), flow=st.sampled_from(Z.FLOWS),
       weighted=st.booleans(), seed=st.integers(0, 1 << 16))
@_pinned(Z.GGC_PINNED)
def test_fuzz_gatedgraphconv_layer(N, deg, loops, C, L, xcols, aggr, bias, flow, weighted, seed):
    """GatedGraphConv(C, L, aggr, bias, flow)(x, edge_index, edge_weight) with x 1-D (xcols = 0), narrower than
    C or C wide: the output and the gradients of x, weight and the GRU cell's parameters against
    tests/_ggc_ref.layer in float64 (the flow's ends swapped for target_to_source).  Pinned (Z.GGC_PINNED): N
    = 1, E = 0, C = 1, C = 128 with a 128-wide x, bias=False with mean."""
    from torch_geometric.nn import GatedGraphConv
    p = dict(N=N, deg=deg, loops=loops, C=C, L=L, xcols=xcols, aggr=aggr, bias=bias, flow=flow, weighted=weighted,
             seed=seed)
    ei, ew, x, gout = Z.ggc_inputs(p)
    what = "N=%d E=%d C=%d L=%d x%s %s bias=%s %s" % (N, ei.shape[1], C, L, tuple(x.shape), aggr, bias, flow)
    torch.manual_seed(seed)
    cpu = GatedGraphConv(C, L, aggr=aggr, bias=bias, flow=flow)
    names = ["x"] + [n for n, _ in cpu.named_parameters()]
    assert ("rnn.bias_ih" in names) == bias
    # float64 reference
    x64 = x.double().requires_grad_(True)
    p64 = [q.detach().double().requires_grad_(True) for q in cpu.parameters()]
    rnn = {n[4:]: q for n, q in zip(names[1:], p64) if n.startswith("rnn.")}
    ends = ei if flow == Z.FLOWS[0] else ei.flip(0)
    ref = _grads(GR.layer(x64 if x64.dim() == 2 else x64.unsqueeze(-1), ends, ew, p64[names.index("weight") - 1], rnn,
                          aggr), gout.double(), [x64] + p64)
    # the recipe in fp32 on the CPU: the bound's `own`
    x32 = x.clone().requires_grad_(True)
    rec = _grads(cpu.recipe(x32, ei, ew), gout, [x32] + list(cpu.parameters()))
    gpu = copy.deepcopy(cpu).to(DEV)
    xd, eid, ewd = x.to(DEV).requires_grad_(True), ei.to(DEV), None if ew is None else ew.to(DEV)
    assert gpu.fused(xd, ewd), what
    out = gpu(xd, eid, ewd, form="fused")
    assert tuple(out.shape) == (N, C), what
    got = _grads(out, gout.to(DEV), [xd] + list(gpu.parameters()))
    worst = 0.0
    for name, g_, r_, c_ in zip(["out"] + names, got, ref, rec):
        assert tuple(g_.shape) == tuple(r_.shape), (name, what)
        own = float((c_.double() - r_).abs().max())
        lim = (1e-5 if name == "out" else 1e-4) * r_.abs().clamp(min=1.0) + 4 * own
        err = (g_.cpu().double() - r_).abs()
        worst = max(worst, float((err / lim).max()))
        assert bool((err <= lim).all()), "%s %s: err %g, fp32 recipe err %g" % (name, what, float(err.max()), own)
    print("GatedGraphConv %s: P = %d, max err / bound %.3g" % (what, K.gru_width(C), worst))


# --------------------------------------------------------------------------
# c. non-contiguous inputs (the sibling of test_fuzz_conv_layer_input_views)
# --------------------------------------------------------------------------

def _view_layer(layer, c_in, flow, seed):
    from torch_geometric.nn import AGNNConv, ARMAConv, GatedGraphConv
    torch.manual_seed(seed)
    if layer == "arma":
        conv, c_out = ARMAConv(c_in, 5, 3, 2, bias=True), 5
        with torch.no_grad():
            for q in conv.bias:
                q.normal_()
    elif layer == "ggc":
        conv, c_out = GatedGraphConv(40, 2, aggr="mean", flow=flow), 40
    else:
        conv, c_out = AGNNConv(flow=flow), c_in
    return conv.to(DEV), c_out


@settings(**_COSTLY)
@given(N=st.integers(1, 80), deg=st.floats(0.0, 8.0), c_in=st.sampled_from([1, 3, 8, 33]),
       layer=st.sampled_from(["arma", "ggc", "agnn"]), xview=st.sampled_from(["offset", "strided", "transposed"]),
       flow=st.sampled_from(Z.FLOWS), seed=st.integers(0, 1 << 16))
@example(N=70, deg=3.0, c_in=33, layer="arma", xview="transposed", flow=Z.FLOWS[0], seed=1)
@example(N=70, deg=3.0, c_in=8, layer="ggc", xview="offset", flow=Z.FLOWS[1], seed=2)
@example(N=40, deg=3.0, c_in=3, layer="agnn", xview="strided", flow=Z.FLOWS[0], seed=3)
@example(N=40, deg=3.0, c_in=8, layer="agnn", xview="offset", flow=Z.FLOWS[1], seed=4)
def test_fuzz_recurrent_layer_input_views(N, deg, c_in, layer, xview, flow, seed):
    """ARMAConv, GatedGraphConv and AGNNConv fed non-contiguous inputs -- x as a column slice at an odd offset, a
    row-strided view and a transposed view, edge_index as the transposed view of an [E, 2] tensor -- give bit
    for bit the output and every gradient of the same call on contiguous clones.  GatedGraphConv's aggregation
    reads the state itself; AGNNConv copies a view once (its kernels choose vec4 or scalar lanes by the rows'
    alignment: while the layer sent a view down the generic path, the pinned c_in = 8 column slice differed from
    its clone by one ulp, 2.4e-7); ARMAConv hands its x-side GEMMs one contiguous x whatever the view, so there
    too the same values meet the same kernels in the same order (agreement to the GEMM's rounding is all the
    layer's contract asks; bitwise holds because of that copy)."""
    ei, g = Z.graph(N, deg, 0.2, seed)
    E = ei.shape[1]
    base = torch.randn(N, c_in, generator=g)
    conv, c_out = _view_layer(layer, c_in, flow, seed)
    gout = torch.randn(N, c_out, generator=g).to(DEV)

    def run(views):
        conv.zero_grad()
        xd = _x_view(base, xview) if views else base.to(DEV).requires_grad_()
        e = ei.t().contiguous().to(DEV).t() if views else ei.to(DEV)
        assert views is False or E < 2 or not e.is_contiguous()
        out = conv(xd, e)
        (out * gout).sum().backward()
        return [("out", out.detach()), ("x", xd.grad)] + [(n, q.grad.clone()) for n, q in conv.named_parameters()
                                                          if q.requires_grad]

    plain, viewed = run(False), run(True)
    assert tuple(plain[0][1].shape) == (N, c_out) and [n for n, _ in plain] == [n for n, _ in viewed]
    for (name, a), (_, b) in zip(plain, viewed):
        assert a is not None and b is not None, name
        assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), name
        assert torch.equal(a, b), "%s %s differs on views by %g" % (layer, name, float((a - b).abs().max()))


# --------------------------------------------------------------------------
# d. empty graphs (the sibling of test_empty_graphs_through_the_fused_conv_layers)
# --------------------------------------------------------------------------

def test_empty_graphs_through_the_recurrent_layers():
    """ARMAConv and GatedGraphConv in both forced forms and the chosen one, AGNNConv and DNAConv, on N in {0, 5}
    nodes without edges: the output is [N, C], the backward runs and d x has x's shape; at N = 5 ARMAConv and
    GatedGraphConv equal their float64 restatements (under the bounds of the two fuzz tests above)."""
    from torch_geometric.nn import AGNNConv, ARMAConv, DNAConv, GatedGraphConv
    ei = torch.empty(2, 0, dtype=torch.long)
    torch.manual_seed(11)
    for N in (0, 5):
        g = torch.Generator().manual_seed(N)
        x = torch.randn(N, 4, generator=g)
        for form in ("fused", "unfused", None):
            conv = ARMAConv(4, 3, 2, 2)
            with torch.no_grad():
                for q in conv.bias:
                    q.normal_()
            ggc = GatedGraphConv(6, 2, aggr="mean")
            for name, layer, c_out in (("ARMAConv", conv, 3), ("GatedGraphConv", ggc, 6)):
                what = "%s %s N=%d E=0" % (name, form, N)
                gpu = copy.deepcopy(layer).to(DEV)
                xd = x.to(DEV).requires_grad_(True)
                out = gpu(xd, ei.to(DEV), form=form)
                assert tuple(out.shape) == (N, c_out), what
                out.sum().backward()
                assert xd.grad is not None and xd.grad.shape == xd.shape, what
                if not N:
                    continue
                if name == "ARMAConv":
                    args = (x, ei, None, [q.detach() for q in layer.ws], [q.detach() for q in layer.vs],
                            [q.detach() for q in layer.bias], 2, False)
                    AR.assert_bound(out, AR.forward(*args)[0], AR.forward(*args, absolute=True)[0], what)
                else:
                    rnn = {n: q.detach() for n, q in layer.rnn.named_parameters()}
                    ref = GR.layer(x, ei, None, layer.weight.detach(), rnn, "mean")
                    own = float((layer.recipe(x, ei).detach().double() - ref).abs().max())
                    err = (out.detach().cpu().double() - ref).abs()
                    assert bool((err <= 1e-5 * ref.abs().clamp(min=1.0) + 4 * own).all()), (what, float(err.max()), own)
        hist = torch.randn(N, 3, 4, generator=g)                        # DNAConv's x: [N, layers, channels]
        for name, gpu, xin, c_out in (("AGNNConv", AGNNConv().to(DEV), x, (N, 4)),
                                      ("DNAConv", DNAConv(4, heads=2).to(DEV), hist, (N, 4))):
            what = "%s N=%d E=0" % (name, N)
            xd = xin.to(DEV).requires_grad_(True)
            out = gpu(xd, ei.to(DEV))
            assert tuple(out.shape) == c_out, what
            out.sum().backward()
            assert xd.grad is not None and xd.grad.shape == xd.shape, what
