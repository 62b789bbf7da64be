"""Layer-level fuzzing of GMMConv on the engine, in the style of
test_gpu_fuzz_conv_layers.py: graphs from tests/_fuzz_cases.py (1..80 nodes, up
to 640 edges: smaller than one wave's rows up to a few blocks, duplicates, self
loops, isolated nodes, no edges at all), the reference the float64 restatement
tests/_gmm_ref.py through the checker of test_gpu_gmm.py.  Every draw is valid
by construction (no assume, no skip).  Each example checks the output shape,
then the forward and every gradient (x, g, mu, sigma, root, bias, and pseudo
when it requires grad) within the project's bound |err| <= 1e-5 * sum |terms|;
without edges d mu, d sigma and d g are exactly zero.  pseudo is uniform in [0,
1] with exact all-0 and all-1 rows; mu and sigma are drawn as in the kernel
tests (|sigma| in [0.5, 1.5)), which keeps an fp32 weight within 1e-6 relative
of float64.
"""
import pytest
import torch
from hypothesis import example, given, settings, strategies as st

from tests import _fuzz_cases as Z
from tests import test_gpu_gmm as TG
from tests.test_gpu_fuzz_layers import _N_EX, _SETTINGS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_COSTLY = dict(_SETTINGS, max_examples=max(10, _N_EX // 2))


def _gm(N, deg, loops, c_in, c_out, K, D, aggr, flow, root, bias, form, p_grad, seed):
    return dict(N=N, deg=deg, loops=loops, c_in=c_in, c_out=c_out, K=K, D=D, aggr=aggr, flow=flow, root=root, bias=bias,
                form=form, p_grad=p_grad, seed=seed)


# N = 1 without edges and with self loops only; E = 0; every edge a loop; mean with isolated nodes; the columns
# mapping with two tiles of k; two column tiles; K * D at the table limit; K above one wave; the gather form at F = 1
PINNED = (
    _gm(1, 0.0, 0.0, 5, 3, 4, 3, "add", Z.FLOWS[0], True, True, None, True, 1),
    _gm(1, 3.0, 1.0, 2, 8, 4, 1, "mean", Z.FLOWS[0], True, True, "bins", True, 2),
    _gm(5, 0.0, 0.0, 5, 3, 4, 3, "add", Z.FLOWS[1], True, True, "gather", False, 3),
    _gm(40, 4.0, 1.0, 16, 3, 25, 2, "add", Z.FLOWS[0], True, False, "gather", True, 4),
    _gm(60, 0.3, 0.0, 5, 33, 4, 1, "mean", Z.FLOWS[1], False, True, "bins", False, 5),
    _gm(50, 4.0, 0.2, 33, 3, 25, 2, "add", Z.FLOWS[0], True, True, "bins", True, 6),
    _gm(50, 4.0, 0.2, 70, 1, 3, 3, "mean", Z.FLOWS[1], True, True, "gather", True, 7),
    _gm(30, 4.0, 0.2, 2, 2, 128, 8, "mean", Z.FLOWS[0], True, True, None, True, 8),
    _gm(30, 4.0, 0.2, 3, 33, 70, 1, "add", Z.FLOWS[0], False, False, "gather", True, 9),
    _gm(70, 6.0, 0.2, 1, 32, 25, 2, "mean", Z.FLOWS[0], True, True, "gather", False, 10),
)


def _pinned(cases):
    def wrap(fn):
        for p in reversed(cases):
            fn = example(**p)(fn)
        return fn
    return wrap


@settings(**_COSTLY)
@given(N=st.integers(1, 80), deg=st.floats(0.0, 8.0), loops=st.sampled_from([0.0, 0.2, 1.0]),
       c_in=st.sampled_from([1, 2, 5, 16, 32, 33, 70]), c_out=st.sampled_from([1, 3, 8, 33, 70]),
       K=st.sampled_from([1, 3, 16, 17, 25]), D=st.sampled_from([1, 2, 3]), aggr=st.sampled_from(["add", "mean"]),
       flow=st.sampled_from(Z.FLOWS), root=st.booleans(), bias=st.booleans(),
       form=st.sampled_from(["bins", "gather", None]), p_grad=st.booleans(), seed=st.integers(0, 1 << 16))
@_pinned(PINNED)
def test_fuzz_gmmconv_layer(N, deg, loops, c_in, c_out, K, D, aggr, flow, root, bias, form, p_grad, seed):
    ei, g = Z.conv_graph(N, deg, loops, seed)
    E = ei.shape[1]
    x = torch.randn(N, c_in, generator=g)
    p = Z.edge_attr(E, D, seed)
    conv = TG._layer(c_in, c_out, K, D, aggr, flow, seed, root_weight=root, bias=bias)
    what = "N=%d E=%d c_in=%d c_out=%d K=%d D=%d %s %s form=%s" % (N, E, c_in, c_out, K, D, aggr, flow, form)
    out, grads = TG.check_layer(conv, x, ei, p, form, what, p_grad=p_grad, seed=seed)
    assert ("root" in grads, "bias" in grads, "pseudo" in grads) == (root, bias, p_grad)
    if E == 0:
        for name in ("mu", "sigma", "g"):
            assert float(grads[name].abs().sum()) == 0.0, "%s: %s is not exactly zero" % (what, name)
        if not root:
            want = conv.bias.detach().expand(N, c_out) if bias else torch.zeros(N, c_out, device=DEV)
            assert torch.equal(out.detach(), want) and float(grads["x"].abs().sum()) == 0.0
