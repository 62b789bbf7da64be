"""Layer-level fuzzing of NNConv and RGCNConv on the engine: the sibling of
test_gpu_fuzz_pool_layers.py for the two fused aggregation families added
after it.

The inputs come from tests/_fuzz_cases.py (shared with the CPU test
tests/test_fuzz_cases_host.py, which runs every pinned example through the
restatements alone); the references are the float64 CPU restatements
tests/_nnconv_ref.py and tests/_rgcn_ref.py through the checkers of
test_gpu_nnconv.py / test_gpu_rgcn.py.  Every draw is valid by construction
(no assume, no skip).  Each test checks the output shape, then the forward
and every gradient within the project's bound |err| <= 1e-5 * sum |terms|;
what no edge reaches (E = 0) is exactly zero; the same call on
non-contiguous views is bitwise the contiguous one.

Graphs have 1..80 nodes and up to 640 edges: smaller than one wave's rows up
to a few blocks, a hub row, duplicates, self loops, isolated nodes.
"""
import pytest
import torch
from hypothesis import example, given, settings, strategies as st

from tests import _fuzz_cases as Z
from tests import test_gpu_nnconv as TN, test_gpu_rgcn as TR
from tests.test_gpu_fuzz_layers import _N_EX, _SETTINGS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_COSTLY = dict(_SETTINGS, max_examples=max(10, _N_EX // 2))
_COSTLIEST = dict(_SETTINGS, max_examples=max(10, _N_EX // 3))


def _pinned(cases):
    """One @example per dict of `cases`."""
    def wrap(fn):
        for p in reversed(cases):
            fn = example(**p)(fn)
        return fn
    return wrap


def _exactly_zero(grads, names, what):
    for name in names:
        assert float(grads[name].abs().sum()) == 0.0, "%s: %s is not exactly zero" % (what, name)


# --------------------------------------------------------------------------
# a. NNConv
# --------------------------------------------------------------------------

def _nnconv_layer(p):
    """The layer of one draw: nn = Linear-ReLU-Linear ("mlp"), or a bare Linear
    ("linear") whose input, edge_attr itself, is h."""
    H, c_in, c_out = p["H"], p["c_in"], p["c_out"]
    torch.manual_seed(p["seed"])
    nn = torch.nn.Linear(H, c_in * c_out, bias=p["head_bias"]) if p["nn"] == "linear" else None
    return TN._layer(c_in, c_out, H, p["aggr"], p["flow"], p["seed"], root=p["root"], bias=p["bias"],
                     head_bias=p["head_bias"], nn=nn, D=p["D"])


@settings(**_COSTLY)
@given(N=st.integers(1, 80), deg=st.floats(0.0, 8.0), loops=st.sampled_from([0.0, 0.2, 1.0]),
       c_in=st.sampled_from([1, 2, 5, 16, 32, 33, 70]), c_out=st.sampled_from([1, 3, 8, 33]),
       H=st.sampled_from([1, 4, 25, 40]), D=st.sampled_from([1, 3]), aggr=st.sampled_from(["add", "mean"]),
       flow=st.sampled_from(Z.FLOWS), root=st.booleans(), bias=st.booleans(), head_bias=st.booleans(),
       form=st.sampled_from(["bins", "gather", None]), nn=st.sampled_from(["mlp", "linear"]),
       seed=st.integers(0, 1 << 16))
@_pinned(Z.NNCONV_PINNED)
def test_fuzz_nnconv_layer(N, deg, loops, c_in, c_out, H, D, aggr, flow, root, bias, head_bias, form, nn, seed):
    """NNConv(c_in, c_out, nn, aggr, flow, root_weight, bias)(x, edge_index,
    edge_attr, form): the output and the gradients of x and of every parameter
    against the float64 restatement; with a bare Linear nn, edge_attr requires
    grad, so the edge-gradient kernel's output is a leaf gradient and is compared
    directly.  Without edges every gradient of the edge network is exactly
    zero.  Pinned (Z.NNCONV_PINNED): N = 1 without edges and with self loops
    only, N = 5 without edges, every edge a loop, mean with isolated nodes, a
    bare Linear at (c_in, H) = (33, 40), (70, 40) and (32, 25), the gather
    form without a head bias."""
    p = dict(N=N, deg=deg, loops=loops, c_in=c_in, c_out=c_out, H=H, D=D, aggr=aggr, flow=flow, root=root, bias=bias,
             head_bias=head_bias, form=form, nn=nn, seed=seed)
    ei, x, ea = Z.nnconv_inputs(p)
    E = ei.shape[1]
    conv = _nnconv_layer(p)
    what = "N=%d E=%d c_in=%d c_out=%d H=%d %s %s %s form=%s" % (N, E, c_in, c_out, H, nn, aggr, flow, form)
    out, grads = TN.check_layer(conv, x, ei, ea, form, what, ea_grad=nn == "linear", seed=seed)
    assert ("edge_attr" in grads) == (nn == "linear")
    assert ("root" in grads, "bias" in grads) == (root, bias)
    assert (("nn.bias" if nn == "linear" else "nn.2.bias") in grads) == head_bias
    if E == 0:
        _exactly_zero(grads, [k for k in grads if k.startswith("nn.") or k == "edge_attr"], what)
        if not root:
            want = conv.bias.detach().expand(N, c_out) if bias else torch.zeros(N, c_out, device=DEV)
            assert torch.equal(out.detach(), want) and float(grads["x"].abs().sum()) == 0.0


# --------------------------------------------------------------------------
# b. RGCNConv
# --------------------------------------------------------------------------

@settings(**_COSTLY)
@given(N=st.integers(1, 80), deg=st.floats(0.0, 8.0), loops=st.sampled_from([0.0, 0.2, 1.0]),
       c_in=st.sampled_from([1, 3, 16, 32, 33, 70]), c_out=st.sampled_from([1, 4, 33, 70]),
       R=st.sampled_from([1, 2, 7, 30]), B=st.sampled_from([1, 2, 5, 17, 65]),
       rkind=st.sampled_from(Z.RELATION_KINDS), nkind=st.sampled_from(Z.NORM_KINDS),
       mode=st.sampled_from(["bins", "gather", "chosen", "featureless"]), flow=st.sampled_from(Z.FLOWS),
       root=st.booleans(), bias=st.booleans(), seed=st.integers(0, 1 << 16))
@_pinned(Z.RGCN_PINNED)
def test_fuzz_rgcnconv_layer(N, deg, loops, c_in, c_out, R, B, rkind, nkind, mode, flow, root, bias, seed):
    """RGCNConv(c_in, c_out, R, B, root_weight, bias, flow)(x, edge_index,
    edge_type, edge_norm, form), featured in both forms and the chosen one, and
    featureless (x = None, in_channels = N): the output and the gradients of
    basis, att, root, bias and (featured) x against the float64 restatement.
    Without edges d att and d basis are exactly zero.  Pinned (Z.RGCN_PINNED): N
    = 1 without edges featured and featureless, N = 5 without edges, R = 1, B =
    65 with three columns, one relation holding more than two chunks of the att
    gradient, every edge a loop, a signed norm."""
    from mi355_mp import ops
    p = dict(N=N, deg=deg, loops=loops, c_in=c_in, c_out=c_out, R=R, B=B, rkind=rkind, nkind=nkind, mode=mode,
             flow=flow, root=root, bias=bias, seed=seed)
    ei, x, et, en = Z.rgcn_inputs(p)
    E = ei.shape[1]
    if rkind == "one" and (N, deg) == (80, 8.0):
        chunk = ops.rgcn_att_chunk()
        assert int(torch.bincount(et).max()) == E > 2 * chunk, (E, chunk)
    conv = TR._layer(N if x is None else c_in, c_out, R, B, flow, seed, root=root, bias=bias)
    form = mode if mode in ("bins", "gather") else None
    what = "N=%d E=%d c_in=%d c_out=%d R=%d B=%d %s %s %s %s" % (N, E, c_in, c_out, R, B, rkind, nkind, mode, flow)
    out, grads = TR._check_layer(conv, x, ei, et, en, form, what)
    assert sorted(grads) == sorted(["att", "basis"] + ["root"] * root + ["bias"] * bias + ["x"] * (x is not None))
    if E == 0:
        _exactly_zero(grads, ["att", "basis"], what)


# --------------------------------------------------------------------------
# c. non-contiguous inputs (the sibling of test_fuzz_pool_layer_input_views)
# --------------------------------------------------------------------------

def _column_of_two(t):
    """t [E] as column 0 of an [E, 2] tensor: the same values at stride 2."""
    return torch.stack([t, torch.flip(t, [0])], dim=1).to(DEV)[:, 0]


def _x_view(base, kind):
    b = base.to(DEV)
    n, F = b.shape
    if kind == "offset":
        big = torch.zeros(n, F + 3, device=DEV)
        big[:, 1:F + 1] = b
        v = big[:, 1:F + 1]
        assert v.stride(0) == F + 3
    elif kind == "strided":
        big = torch.zeros(2 * n, F, device=DEV)
        big[::2] = b
        v = big[::2]                                                  # every second row
        assert v.stride(0) == 2 * F
    else:
        assert kind == "transposed"
        v = b.t().contiguous().t()
    assert torch.equal(v, b)
    return v.detach().requires_grad_()


@settings(**_COSTLY)
@given(N=st.integers(1, 80), deg=st.floats(0.0, 8.0), c_in=st.sampled_from([1, 3, 8, 33]),
       layer=st.sampled_from(["nnconv_mlp", "nnconv_linear", "rgcn"]), form=st.sampled_from(["bins", "gather"]),
       xview=st.sampled_from(["offset", "strided", "transposed"]), flow=st.sampled_from(Z.FLOWS),
       seed=st.integers(0, 1 << 16))
@example(N=70, deg=3.0, c_in=33, layer="nnconv_linear", form="bins", xview="transposed", flow=Z.FLOWS[0], seed=1)
@example(N=70, deg=3.0, c_in=8, layer="rgcn", form="gather", xview="offset", flow=Z.FLOWS[1], seed=2)
@example(N=40, deg=3.0, c_in=3, layer="nnconv_mlp", form="gather", xview="strided", flow=Z.FLOWS[0], seed=3)
def test_fuzz_conv_layer_input_views(N, deg, c_in, layer, form, xview, flow, seed):
    """NNConv and RGCNConv fed non-contiguous inputs -- x as a column slice at an
    odd offset, a row-strided view and a transposed view, edge_index as the
    transposed view of an [E, 2] tensor, a bare Linear's edge_attr as a column
    slice of a wider tensor, edge_type and edge_norm as one column of [E, 2]
    tensors -- give bit for bit the output and every gradient (x, the
    parameters, edge_attr) of the same call on contiguous clones: the kernels
    are deterministic and see the same values in the same order, and the layers
    hand their GEMMs (x root, x L') one contiguous x whatever the view.  Pinned: a
    transposed x through NNConv's x root, which differed by one ulp (4.8e-7)
    while the layer passed the view on to the GEMM."""
    ei, g = Z.graph(N, deg, 0.2, seed)
    E = ei.shape[1]
    base = torch.randn(N, c_in, generator=g)
    c_out, H = 4, 5
    linear = layer == "nnconv_linear"
    torch.manual_seed(seed)
    if layer == "rgcn":
        conv = TR._layer(c_in, c_out, 3, 5, flow, seed).to(DEV)
        et, en = Z.relations("uniform", E, 3, seed), Z.edge_norm("rand", E, seed)
    else:
        D = H if linear else 2
        nn = torch.nn.Linear(H, c_in * c_out) if linear else None
        conv = TN._layer(c_in, c_out, H, "mean", flow, seed, nn=nn, D=D).to(DEV)
        ea = Z.edge_attr(E, D, seed)
    gout = torch.randn(N, c_out, generator=g).to(DEV)

    def args(views):
        xd = _x_view(base, xview) if views else base.to(DEV).requires_grad_()
        e = ei.t().contiguous().to(DEV).t() if views else ei.to(DEV)
        assert views is False or E < 2 or not e.is_contiguous()
        if layer == "rgcn":
            rest = (_column_of_two(et), _column_of_two(en)) if views else (et.to(DEV), en.to(DEV))
            assert not views or E < 2 or rest[0].stride(0) == rest[1].stride(0) == 2
            return xd, e, rest, None
        if views and linear:                                          # (an mlp's trunk is torch's own Linear)
            big = torch.zeros(E, ea.shape[1] + 3, device=DEV)
            big[:, 1:ea.shape[1] + 1] = ea.to(DEV)
            ead = big[:, 1:ea.shape[1] + 1].detach()
            assert E == 0 or ead.stride(0) == ea.shape[1] + 3
        else:
            ead = ea.to(DEV)
        ead.requires_grad_(linear)
        return xd, e, (ead,), ead

    def run(views):
        conv.zero_grad()
        xd, e, rest, ead = args(views)
        out = conv(xd, e, *rest, form=form)
        (out * gout).sum().backward()
        got = [("out", out.detach()), ("x", xd.grad)] + [(n, p.grad.clone()) for n, p in conv.named_parameters()]
        if linear:
            got.append(("edge_attr", ead.grad))
        return got

    plain, viewed = run(False), run(True)
    assert tuple(plain[0][1].shape) == (N, c_out) and [n for n, _ in plain] == [n for n, _ in viewed]
    for (name, a), (_, b) in zip(plain, viewed):
        assert a is not None and b is not None, name
        assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), name
        assert torch.equal(a, b), "%s differs on views by %g" % (name, float((a - b).abs().max()))
