"""GPU tests of the dense family (csrc/mp_dense.hip): the raw entry points on
NaN-filled outputs against the float64 restatement (tests/_dense_ref.py) over the
shapes of tests/_dense_cases.py, run-to-run bit identity, the exact to_dense_*
fills, and the layers through autograd on both the fused and the recipe branch.

Bounds (tests/_dense_cases.py): arrays |got - want| <= 1e-4 max(1, |want|); the
two losses relative, four times the fp32 upstream recipe's own worst relative
error against float64 on these shapes on the CPU (measured 7.9e-7, so 3.2e-6),
capped at 1e-4."""
import numpy as np
import pytest
import torch

from tests import _dense_cases as K
from tests import _dense_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def env():
    import mi355_mp
    from mi355_mp import _lib, ops
    mi355_mp.load_native()
    return _lib.native(), _lib, ops


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _raw_forward(nat, _lib, t):
    """mp_dense_diff_pool_f32 on NaN-filled outputs: dict of device tensors and the launches."""
    x, adj, s = (t[k].to(DEV).contiguous() for k in ("x", "adj", "s"))
    B, N, F = x.shape
    C = s.shape[2]
    mask = None if t["mask"] is None else t["mask"].to(torch.uint8).to(DEV)
    o = {"out": _nan(B, C, F), "out_adj": _nan(B, C, C), "loss": _nan(4), "P": _nan(B, N, C), "T": _nan(B, N, C),
         "V": _nan(B, N, C)}
    wsb = nat.mp_diff_pool_workspace(B, N, C, F)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=DEV)      # NaN bit patterns in the partials too
    rc = nat.mp_dense_diff_pool_f32(x.data_ptr(), adj.data_ptr(), s.data_ptr(), _lib.ptr(mask), B, N, C, F,
                                    o["out"].data_ptr(), _lib.nbytes(o["out"]), o["out_adj"].data_ptr(),
                                    _lib.nbytes(o["out_adj"]), o["loss"].data_ptr(), 16, o["P"].data_ptr(),
                                    _lib.nbytes(o["P"]), o["T"].data_ptr(), _lib.nbytes(o["T"]), o["V"].data_ptr(),
                                    _lib.nbytes(o["V"]), ws.data_ptr(), wsb, _lib.stream_ptr(DEV))
    assert rc > 0, nat.mp_last_error()
    torch.cuda.synchronize()
    o.update(x=x, adj=adj, s=s, mask=mask, launches=rc)
    return o


def _raw_backward(nat, _lib, o, g_out, g_oa, gl, ge, want_dx=True):
    B, N, F = o["x"].shape
    C = o["s"].shape[2]
    g_out = None if g_out is None else g_out.to(DEV).contiguous()
    g_oa = None if g_oa is None else g_oa.to(DEV).contiguous()
    g_loss = None if gl is None else torch.tensor([gl, ge], dtype=torch.float32, device=DEV)
    dx, ds = (_nan(B, N, F) if want_dx else None), _nan(B, N, C)
    wsb = nat.mp_diff_pool_bwd_workspace(B, N, C, F)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=DEV)
    rc = nat.mp_dense_diff_pool_bwd_f32(_lib.ptr(g_out), _lib.ptr(g_oa), _lib.ptr(g_loss), o["x"].data_ptr(),
                                        o["P"].data_ptr(), o["T"].data_ptr(), o["V"].data_ptr(), o["loss"].data_ptr(),
                                        B, N, C, F, _lib.ptr(dx), _lib.nbytes(dx), ds.data_ptr(), _lib.nbytes(ds),
                                        ws.data_ptr(), wsb, _lib.stream_ptr(DEV))
    assert rc > 0, nat.mp_last_error()
    torch.cuda.synchronize()
    return dx, ds


def _cases():
    return K.diff_pool_cases(K.path_twin)


def pytest_generate_tests(metafunc):
    if "case" in metafunc.fixturenames:
        cases = _cases()
        metafunc.parametrize("case", cases, ids=["B%d-N%d-C%d-F%d-%s-%s" % c for c in cases])


def test_diff_pool_raw_forward_and_backward(env, case):
    """Every output against float64; no NaN of the fill survives; the second run is the same bits."""
    nat, _lib, ops = env
    assert _cases() == K.diff_pool_cases(ops.diff_pool_path)          # the collected list is the native query's
    t = K.diff_pool_inputs(case)
    B, N, C, F = case[:4]
    o = _raw_forward(nat, _lib, t)
    assert o["launches"] == (2 if ops.diff_pool_path(N, C, F) == 0 else 8)
    want = R.diff_pool(t["x"], t["adj"], t["s"], t["mask"])
    errs = {k: K.close(o[k], want[k]) for k in ("out", "out_adj", "P", "T", "V")}
    link, ent, qs, hs = o["loss"].tolist()
    e_link, e_ent = K.loss_err(link, want["link"]), K.loss_err(ent, want["ent"], K.ENT_FLOOR)
    e_q = K.loss_err(qs, want["q"].sum())
    print(case, {k: "%.2g" % v for k, v in errs.items()}, "link %.2g ent %.2g q %.2g" % (e_link, e_ent, e_q))
    assert max(errs.values()) <= K.ARRAY_TOL, errs
    assert e_link <= K.LOSS_RTOL and e_ent <= K.LOSS_RTOL and e_q <= 2 * K.LOSS_RTOL, (e_link, e_ent, e_q)
    assert K.close(torch.tensor(hs), want["h"].sum()) <= K.ARRAY_TOL
    if t["mask"] is not None:
        dead = ~t["mask"].to(DEV)
        assert float(o["P"][dead].abs().max() if dead.any() else 0.0) == 0.0       # padding rows are exactly zero
    # backward: all terms, then the link term alone at a weight that makes it O(1)
    dx, ds = _raw_backward(nat, _lib, o, t["g_out"], t["g_oa"], t["gl"], t["ge"])
    g = R.diff_pool_grads(t["x"], t["adj"], t["s"], t["mask"], t["g_out"], t["g_oa"], t["gl"], t["ge"])
    e_dx, e_ds = K.close(dx, g["dx"]), K.close(ds, g["ds"])
    gl = float(B * N * N)
    _, ds_l = _raw_backward(nat, _lib, o, None, None, gl, 0.0, want_dx=False)
    zero_o, zero_a = torch.zeros(B, C, F), torch.zeros(B, C, C)
    if float(want["q"].sum()) > 0:
        g_l = R.diff_pool_grads(t["x"], t["adj"], t["s"], t["mask"], zero_o, zero_a, gl, 0.0)["ds"]
    else:
        g_l = torch.zeros(B, N, C, dtype=torch.float64)
    e_l = K.close(ds_l, g_l)
    print("   dx %.2g ds %.2g ds(link) %.2g" % (e_dx, e_ds, e_l))
    assert max(e_dx, e_ds, e_l) <= K.ARRAY_TOL
    # bit identity, forward and backward
    o2 = _raw_forward(nat, _lib, t)
    for k in ("out", "out_adj", "loss", "P", "T", "V"):
        assert torch.equal(o[k], o2[k]), k
    dx2, ds2 = _raw_backward(nat, _lib, o2, t["g_out"], t["g_oa"], t["gl"], t["ge"])
    assert torch.equal(dx, dx2) and torch.equal(ds, ds2)


def test_diff_pool_zero_residual_and_missing_gradients(env):
    """q = 0 (adj = P P^T: one node, one cluster): link = 0, k = 0, no NaN; NULL
    gradients are zero terms; dx = NULL is not written."""
    nat, _lib, ops = env
    t = {"x": torch.randn(2, 1, 3), "adj": torch.ones(2, 1, 1), "s": torch.randn(2, 1, 1), "mask": None}
    o = _raw_forward(nat, _lib, t)
    assert o["loss"].tolist()[0] == 0.0 and o["loss"].tolist()[2] == 0.0
    g_out = torch.randn(2, 1, 3)
    dx, ds = _raw_backward(nat, _lib, o, g_out, None, 3.0, 0.5)
    want = R.diff_pool_grads(t["x"], t["adj"], t["s"], None, g_out, torch.zeros(2, 1, 1), 0.0, 0.5)
    assert K.close(dx, want["dx"]) <= K.ARRAY_TOL and K.close(ds, want["ds"]) <= K.ARRAY_TOL
    t = K.diff_pool_inputs((3, 70, 5, 4, "01", "part"))
    o = _raw_forward(nat, _lib, t)
    dx, ds = _raw_backward(nat, _lib, o, None, None, None, None)
    assert float(dx.abs().max()) == 0.0 and float(ds.abs().max()) == 0.0
    dx, ds = _raw_backward(nat, _lib, o, None, t["g_oa"], None, None, want_dx=False)
    want = R.diff_pool_grads(t["x"], t["adj"], t["s"], t["mask"], torch.zeros(3, 5, 4), t["g_oa"], 0.0, 0.0)
    assert dx is None and K.close(ds, want["ds"]) <= K.ARRAY_TOL


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 2, 3), (20, 63, 64), (1, 64, 65), (3, 65, 192), (3, 100, 1),
                                   (2, 129, 33)])
@pytest.mark.parametrize("add_loop", [False, True])
def test_dense_mean_agg_raw(env, shape, add_loop):
    nat, _lib, ops = env
    B, N, F = shape
    g = torch.Generator().manual_seed(B + N + F)
    x = torch.randn(B, N, F, generator=g)
    for kind in K.ADJ_KINDS:
        adj = K.make_adj(kind, B, N, g)
        xd, ad = x.to(DEV), adj.to(DEV)
        keep = ad.clone()
        out, deg = _nan(B, N, F), _nan(B, N)
        rc = nat.mp_dense_mean_agg_f32(ad.data_ptr(), xd.data_ptr(), B, N, F, int(add_loop), 0, None, out.data_ptr(),
                                       _lib.nbytes(out), deg.data_ptr(), _lib.nbytes(deg), _lib.stream_ptr(DEV))
        assert rc == 1, nat.mp_last_error()
        want, wdeg = R.mean_agg(x, adj, add_loop)
        assert K.close(out, want) <= K.ARRAY_TOL and K.close(deg, wdeg) <= K.ARRAY_TOL
        assert torch.equal(ad, keep)                                  # adj is read, never written
        gy = torch.randn(B, N, F, generator=g)
        dx = _nan(B, N, F)
        rc = nat.mp_dense_mean_agg_f32(ad.data_ptr(), gy.to(DEV).data_ptr(), B, N, F, int(add_loop), 1, deg.data_ptr(),
                                       dx.data_ptr(), _lib.nbytes(dx), None, 0, _lib.stream_ptr(DEV))
        assert rc == 1, nat.mp_last_error()
        xr = x.double().requires_grad_(True)
        (R.mean_agg(xr, adj, add_loop)[0] * gy.double()).sum().backward()
        assert K.close(dx, xr.grad) <= K.ARRAY_TOL
        out2 = _nan(B, N, F)
        nat.mp_dense_mean_agg_f32(ad.data_ptr(), xd.data_ptr(), B, N, F, int(add_loop), 0, None, out2.data_ptr(),
                                  _lib.nbytes(out2), deg.data_ptr(), _lib.nbytes(deg), _lib.stream_ptr(DEV))
        assert torch.equal(out, out2)


@pytest.mark.parametrize("sizes", [[3, 1, 4], [0, 2, 5], [2, 0, 0, 5], [2, 5, 0, 0], [70, 3, 129]])
def test_to_dense_fills_are_exact(env, sizes):
    """Graphs without nodes first, in the middle and last (a layout extended past
    the last node), duplicate edges, a non-zero fill value; the gather backward."""
    nat, _lib, ops = env
    from torch_geometric.utils import to_dense_adj, to_dense_batch
    G, n = len(sizes), sum(sizes)
    starts = [0] + list(np.cumsum(sizes))
    g = torch.Generator().manual_seed(n + G)
    batch = torch.repeat_interleave(torch.arange(G), torch.tensor(sizes)).to(DEV)
    layout = ops.cached_batch_layout_for(batch, n, G, torch.device(DEV))
    assert layout.n_graphs == G and layout.max_n == max(sizes)
    x = torch.randn(n, 5, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    out, mask = ops.to_dense_batch(xd, layout, -2.5)
    want, wmask = R.to_dense_batch(x, starts, -2.5)
    assert torch.equal(out.detach().cpu(), want) and torch.equal(mask.cpu(), wmask) and mask.dtype == torch.bool
    gd = torch.randn(out.shape, generator=g)
    if n:
        (out * gd.to(DEV)).sum().backward()
        assert torch.equal(xd.grad.cpu(), gd[wmask])                  # the row gather
    if n == 0:
        return
    parts = [torch.randint(0, s, (2, 3 * s + 2), generator=g) + starts[i] for i, s in enumerate(sizes) if s > 0]
    ei = torch.cat(parts + parts[:1], dim=1)                          # the first graph's edges twice: duplicates
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    attr = torch.randn(ei.shape[1], 3, generator=g)
    got = ops.to_dense_adj(ei.to(DEV), layout, batch)
    assert torch.equal(got.cpu(), R.to_dense_adj(ei, starts, batch.cpu()))
    got = ops.to_dense_adj(ei.to(DEV), layout, batch, attr.to(DEV))
    assert torch.equal(got.cpu(), R.to_dense_adj(ei, starts, batch.cpu(), attr))   # the last edge of a cell wins
    assert torch.equal(got, ops.to_dense_adj(ei.to(DEV), layout, batch, attr.to(DEV)))
    # the public functions see the graphs up to the last node
    B = int(batch.max()) + 1
    o2, m2 = to_dense_batch(x.to(DEV), batch, fill_value=-2.5)
    assert torch.equal(o2.cpu(), want[:B]) and torch.equal(m2.cpu(), wmask[:B])
    assert torch.equal(to_dense_adj(ei.to(DEV), batch, attr[:, 0].to(DEV)).cpu(),
                       R.to_dense_adj(ei, starts[:B + 1], batch.cpu(), attr[:, :1])[..., 0])
    perm = torch.randperm(n, generator=g)                             # an unsorted batch takes the recipe
    o3, m3 = to_dense_batch(x[perm].to(DEV), batch[perm.to(DEV)])
    assert m3.sum(-1).tolist() == sizes[:B] and o3.shape == (B, max(sizes), 5)


def _f64(module):
    import copy
    return copy.deepcopy(module).cpu().double()


@pytest.mark.parametrize("shape", [(3, 40, 6, 5), (2, 150, 12, 7)])
def test_layers_through_autograd_on_both_branches(env, shape, monkeypatch):
    """DenseSAGEConv and dense_diff_pool, fused (adj without a gradient) and recipe
    (adj requires one), forward and gradients against float64 autograd."""
    from torch_geometric.nn import DenseSAGEConv, dense_diff_pool
    from torch_geometric.nn.dense import _dense
    B, N, C, F = shape
    t = K.diff_pool_inputs((B, N, C, F, "01", "part"))
    conv = DenseSAGEConv(F, C, normalize=True).to(DEV)
    ref = _f64(conv)
    for adj_grad, forced in ((False, False), (True, False), (False, True)):
        if forced:                                                    # the fused calls whatever the layers would pick
            monkeypatch.setattr(_dense, "pool_fused", lambda x, adj, s: x.is_cuda)   # (the float64 reference runs on the host)
            monkeypatch.setattr(_dense, "agg_fused", lambda x, adj: x.is_cuda)
        x = t["x"].to(DEV).requires_grad_(True)
        adj = t["adj"].to(DEV).requires_grad_(adj_grad)
        mask = t["mask"].to(DEV)
        assert _dense.fused(adj, x) == (not adj_grad)
        assert forced or _dense.agg_fused(x, adj) == (not adj_grad and N <= 128)
        conv.zero_grad()
        s = conv(x, adj, mask)
        assert forced or _dense.pool_fused(x, adj, s) == (not adj_grad and N <= 128)   # beyond: the recipe
        out, out_adj, link, ent = dense_diff_pool(x, adj, s, mask)
        obj = (out * t["g_out"].to(DEV)).sum() + (out_adj * t["g_oa"].to(DEV)).sum() + 500.0 * link + ent
        obj.backward()
        xr = t["x"].double().requires_grad_(True)
        ar = t["adj"].double().requires_grad_(adj_grad)
        ref.zero_grad()
        sr = ref(xr, ar, t["mask"])
        r = R.diff_pool(xr, ar, sr, t["mask"])
        (((r["out"] * t["g_out"].double()).sum() + (r["out_adj"] * t["g_oa"].double()).sum() + 500.0 * r["link"]
          + r["ent"])).backward()
        assert K.close(s, sr) <= K.ARRAY_TOL and K.close(out, r["out"]) <= K.ARRAY_TOL
        assert K.close(out_adj, r["out_adj"]) <= K.ARRAY_TOL
        assert K.loss_err(link, r["link"]) <= K.LOSS_RTOL and K.loss_err(ent, r["ent"], K.ENT_FLOOR) <= K.LOSS_RTOL
        assert K.close(x.grad, xr.grad) <= K.ARRAY_TOL
        assert K.close(conv.weight.grad, ref.weight.grad) <= K.ARRAY_TOL
        assert K.close(conv.bias.grad, ref.bias.grad) <= K.ARRAY_TOL
        if adj_grad:
            assert K.close(adj.grad, ar.grad) <= K.ARRAY_TOL


def test_two_level_stack_reaches_the_first_pool_network(env):
    """The second level's adjacency is the first level's out_adj and requires a
    gradient: it takes the recipe, and the first pool network's parameters get
    their gradient through it."""
    from torch_geometric.nn import DenseSAGEConv, dense_diff_pool
    from torch_geometric.nn.dense import _dense
    B, N, F, C1, C2 = 4, 30, 5, 6, 3
    t = K.diff_pool_inputs((B, N, C1, F, "01", "part"))
    torch.manual_seed(3)
    pool1, embed1 = DenseSAGEConv(F, C1).to(DEV), DenseSAGEConv(F, 8).to(DEV)
    pool2, embed2 = DenseSAGEConv(8, C2).to(DEV), DenseSAGEConv(8, 8).to(DEV)
    mods = (pool1, embed1, pool2, embed2)
    refs = [_f64(m) for m in mods]

    def run(mods, x, adj, mask, pool, check=None):
        pool1, embed1, pool2, embed2 = mods
        s = pool1(x, adj, mask)
        h = embed1(x, adj, mask).relu()
        x1, adj1, l1, e1 = pool(h, adj, s, mask)
        if check:
            check(adj, adj1)
        s2 = pool2(x1, adj1)
        h2 = embed2(x1, adj1).relu()
        x2, adj2, l2, e2 = pool(h2, adj1, s2)
        return x2.sum() + adj2.sum() + 100.0 * (l1 + l2) + e1 + e2

    def check(adj, adj1):
        assert _dense.agg_fused(adj, adj) and adj1.requires_grad and not _dense.fused(adj1, adj1)

    obj = run(mods, t["x"].to(DEV), t["adj"].to(DEV), t["mask"].to(DEV), dense_diff_pool, check)
    obj.backward()

    def pool64(x, adj, s, mask=None):
        r = R.diff_pool(x, adj, s, mask)
        return r["out"], r["out_adj"], r["link"], r["ent"]
    want = run(refs, t["x"].double(), t["adj"].double(), t["mask"], pool64)
    want.backward()
    assert K.close(obj, want) <= K.ARRAY_TOL
    for m, r in zip(mods, refs):
        assert m.weight.grad is not None and float(m.weight.grad.abs().max()) > 0
        assert K.close(m.weight.grad, r.weight.grad) <= K.ARRAY_TOL
        assert K.close(m.bias.grad, r.bias.grad) <= K.ARRAY_TOL
