"""CPU tests of the dense family (DiffPool, DenseSAGEConv, to_dense_*): the
float64 restatement (tests/_dense_ref.py) against its literal per-entry loops
and the committed known answers, the fused backward's formulas against float64
autograd, masks, the q = 0 corner, the path query, the fp32 recipe's own error
on the GPU tests' shapes (it sets their loss bound), ToDense, DenseDataLoader,
to_dense_* on host tensors, the layers' fused / recipe choice, and the C-ABI's
rejection of every bad argument (a C harness under the host-ASAN build of the
library, run as a plain program)."""
import importlib.util
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import _dense_cases as K
from tests import _dense_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch_geometric-1_amd", "csrc")
LIB = os.path.join(ROOT, "pytorch_geometric-1_amd", "mi355_mp", "libmi355_mp.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j4", "-C", CSRC])
    from mi355_mp import _lib
    return _lib.load()


def _golden():
    spec = importlib.util.spec_from_file_location("make_golden_dense",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_dense.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk, np.load(os.path.join(ROOT, "tests", "golden", "dense", "dense_kat.npz"))


@pytest.mark.parametrize("mask_kind", K.MASK_KINDS)
@pytest.mark.parametrize("adj_kind", K.ADJ_KINDS)
def test_restatement_is_the_per_entry_loop(mask_kind, adj_kind):
    """mask = None, a full graph beside padded ones, and a graph whose nodes are all masked."""
    t = K.diff_pool_inputs((3, 5, 3, 2, adj_kind, mask_kind))
    got, want = R.diff_pool(t["x"], t["adj"], t["s"], t["mask"]), R.diff_pool_loop(t["x"], t["adj"], t["s"], t["mask"])
    for k in want:
        assert got[k].dtype == torch.float64 and got[k].shape == want[k].shape, k
        assert float((got[k] - want[k]).abs().max()) <= 1e-13, k
    if mask_kind == "empty_graph":
        assert float(got["P"][0].abs().max()) == 0.0 and float(got["out"][0].abs().max()) == 0.0
        assert float(got["out_adj"][0].abs().max()) == 0.0 and float(got["h"][0]) == 0.0
        assert abs(float(got["q"][0]) - float((t["adj"][0].double() ** 2).sum())) <= 1e-12   # padding counts in q
    if mask_kind is None:
        assert float((got["P"].sum(-1) - 1).abs().max()) <= 1e-12
    for loop in (False, True):
        a, d = R.mean_agg(t["x"], t["adj"], loop)
        al, dl = R.mean_agg_loop(t["x"], t["adj"], loop)
        assert float((a - al).abs().max()) <= 1e-13 and float((d - dl).abs().max()) <= 1e-13


def test_restatement_hand_values():
    """Two nodes, s rows (0, ln 3): P = (1/4, 3/4); the rest is worked in make_golden_dense.py."""
    mk, kat = _golden()
    t, want = mk.hand()
    r = R.diff_pool(t["hand.x"], t["hand.adj"], t["hand.s"])
    assert torch.allclose(r["P"], torch.tensor([[[0.25, 0.75], [0.25, 0.75]]], dtype=torch.float64), atol=1e-12)
    assert r["out"].reshape(-1).tolist() == pytest.approx([3.0, 9.0], abs=1e-12)
    assert float(r["q"][0]) == pytest.approx(17.0 / 16.0, abs=1e-12)
    assert float(r["link"]) == pytest.approx(math.sqrt(17.0) / 16.0, abs=1e-12)
    assert float(r["ent"]) == pytest.approx(math.log(4.0) - 0.75 * math.log(3.0), abs=1e-12)
    for k, v in want.items():
        assert np.abs(r[k.split(".out.")[1]].numpy() - kat[k]).max() <= 1e-12, k      # and the committed copy of it
        assert np.abs(v.numpy() - kat[k]).max() == 0.0, k
    out, out_adj, link, ent = R.diff_pool_recipe(t["hand.x"].double(), t["hand.adj"].double(), t["hand.s"].double())
    assert float((out - r["out"]).abs().max()) <= 1e-12 and float((out_adj - r["out_adj"]).abs().max()) <= 1e-12
    assert abs(float(link - r["link"])) <= 1e-12 and abs(float(ent - r["ent"])) <= 1e-12


def test_restatement_matches_the_committed_known_answers():
    mk, kat = _golden()
    t = {k: torch.from_numpy(kat[k]) for k in mk.inputs()}
    for k, v in mk.inputs().items():
        assert torch.equal(t[k], v), k                              # the generator still draws the committed inputs
    got = mk.answers(t, R.diff_pool, R.mean_agg)
    assert len(got) == (len(mk.KEYS) + 4) * len(mk.CASES)
    for k, v in got.items():
        assert v.dtype == torch.float64 and np.abs(v.numpy() - kat[k]).max() <= 1e-13, k


@pytest.mark.parametrize("mask_kind", K.MASK_KINDS)
def test_gradient_formulas_match_float64_autograd(mask_kind):
    """dP, ds and dx as include/mi355_mp.h states them, from P, T, V and sum q alone."""
    for adj_kind in K.ADJ_KINDS:
        t = K.diff_pool_inputs((3, 6, 4, 5, adj_kind, mask_kind), seed=1)
        r = R.diff_pool(t["x"], t["adj"], t["s"], t["mask"])
        want = R.diff_pool_grads(t["x"], t["adj"], t["s"], t["mask"], t["g_out"], t["g_oa"], t["gl"], t["ge"])
        dx, ds = R.diff_pool_backward(t["x"], t["mask"], r["P"], r["T"], r["V"], r["q"].sum(), t["g_out"], t["g_oa"],
                                      t["gl"], t["ge"])
        assert float((dx - want["dx"]).abs().max()) <= 1e-12 and float((ds - want["ds"]).abs().max()) <= 1e-12
        if mask_kind == "empty_graph":
            assert float(ds[0].abs().max()) == 0.0 and float(dx[0].abs().max()) == 0.0


def test_zero_residual_gives_a_zero_link_gradient_and_no_nan():
    """adj = P P^T exactly (one node, one cluster: P = 1, adj = 1): sqrt has no
    derivative at 0 and autograd returns NaN there; the formulas take k = 0."""
    x, adj, s = torch.randn(2, 1, 3).double(), torch.ones(2, 1, 1).double(), torch.randn(2, 1, 1).double()
    r = R.diff_pool(x, adj, s)
    assert float(r["q"].sum()) == 0.0 and float(r["link"]) == 0.0
    g_out, g_oa = torch.randn(2, 1, 3).double(), torch.randn(2, 1, 1).double()
    dx, ds = R.diff_pool_backward(x, None, r["P"], r["T"], r["V"], r["q"].sum(), g_out, g_oa, 3.0, 0.5)
    dx0, ds0 = R.diff_pool_backward(x, None, r["P"], r["T"], r["V"], r["q"].sum(), g_out, g_oa, 0.0, 0.5)
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(ds).all())
    assert torch.equal(dx, dx0) and torch.equal(ds, ds0)
    want = R.diff_pool_grads(x, adj, s, None, g_out, g_oa, 0.0, 0.5)
    assert float((dx - want["dx"]).abs().max()) <= 1e-12 and float((ds - want["ds"]).abs().max()) <= 1e-12


def test_path_query(lib):
    from mi355_mp import ops
    for C in (1, 3, 10, 33, 64, 65, 200, 5000):
        paths = [lib.mp_diff_pool_path(n, C, 7) for n in list(range(1, 400)) + [1000, 1 << 14, 1 << 20]]
        assert paths == sorted(paths) and paths[-1] == 1, C              # monotone in N, the tiled form reached
        assert paths[0] == 0                                             # and one workgroup at the small end
        assert ops.diff_pool_path(40, C, 7) == lib.mp_diff_pool_path(40, C, 7)
        assert paths == [K.path_twin(n, C, 7) for n in list(range(1, 400)) + [1000, 1 << 14, 1 << 20]]
        for F in (1, 192):
            assert lib.mp_diff_pool_path(100, C, F) == lib.mp_diff_pool_path(100, C, 7)
    assert lib.mp_diff_pool_path(100, 10, 192) == 0                        # the example's first level: one workgroup
    assert lib.mp_diff_pool_path(128, 10, 3) == 0 and lib.mp_diff_pool_path(129, 10, 3) == 1
    assert lib.mp_diff_pool_path(1000, 100, 64) == 1
    assert len(K.boundaries(lib.mp_diff_pool_path, 10)) == 3 and len(K.boundaries(lib.mp_diff_pool_path, 64)) == 3
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 3, 3)):
        assert lib.mp_diff_pool_path(*bad) == -1 and b"mp_diff_pool_path" in lib.mp_last_error()   # -MP_ERR_ARG
        with pytest.raises(ValueError):
            ops.diff_pool_path(*bad)
    # the workspace follows the form: tile partials and row entropies only beyond one workgroup
    assert lib.mp_diff_pool_workspace(20, 100, 10, 192) == 5 * 256
    assert lib.mp_diff_pool_workspace(32, 1000, 100, 64) >= (32 * 16 * 16 + 32 * 1000) * 4
    assert lib.mp_diff_pool_bwd_workspace(32, 1000, 100, 64) >= 32 * 100 * 100 * 4


def test_fp32_recipe_sets_the_loss_bound(lib):
    """The fp32 upstream recipe on the CPU against float64 over the GPU tests'
    shapes and inputs: its arrays stay within the array bound (so the bound is a
    fair one for honest fp32 on randn inputs at unit scale), and its worst
    relative loss error is what tests/_dense_cases.py records (the GPU tests
    allow four times that)."""
    cases = K.diff_pool_cases(lib.mp_diff_pool_path)
    assert len(cases) >= 20 and {c[4] for c in cases} == set(K.ADJ_KINDS) and {c[5] for c in cases} == set(K.MASK_KINDS)
    assert {c[1] for c in cases} >= {1, 2, 63, 64, 65, 100, 127, 128, 129}
    assert {c[2] for c in cases} == {1, 3, 10, 33, 64, 65} and {c[3] for c in cases} == {1, 3, 64, 65, 192}
    assert {c[0] for c in cases} == {1, 3, 20} and {lib.mp_diff_pool_path(c[1], c[2], c[3]) for c in cases} == {0, 1}
    worst_arr, worst_loss = 0.0, 0.0
    for case in cases:
        t = K.diff_pool_inputs(case)
        want = R.diff_pool(t["x"], t["adj"], t["s"], t["mask"])
        out, out_adj, link, ent = R.diff_pool_recipe(t["x"], t["adj"], t["s"], t["mask"])
        assert out.dtype == torch.float32
        worst_arr = max(worst_arr, K.close(out, want["out"]), K.close(out_adj, want["out_adj"]))
        worst_loss = max(worst_loss, K.loss_err(link, want["link"]), K.loss_err(ent, want["ent"], K.ENT_FLOOR))
        assert case[2] == 1 or float(want["ent"]) > 0.3                 # only C = 1 comes near the entropy's floor
    print("fp32 recipe: worst array error %.3g (bound %g), worst relative loss error %.3g" %
          (worst_arr, K.ARRAY_TOL, worst_loss))
    assert worst_arr <= K.ARRAY_TOL
    assert worst_loss <= K.RECIPE_LOSS_ERR and K.LOSS_RTOL == min(4 * K.RECIPE_LOSS_ERR, 1e-4)
    assert worst_loss >= K.RECIPE_LOSS_ERR / 4                          # the recorded figure is the measured one, not a loose cap


def test_to_dense_transform_and_loader():
    import torch_geometric.transforms as T
    from torch_geometric.data import Data, DenseDataLoader
    ei = torch.tensor([[0, 1, 2, 2], [1, 0, 0, 2]])
    d = Data(x=torch.arange(6.0).view(3, 2), edge_index=ei, pos=torch.ones(3, 3), y=torch.tensor([1, 2, 3]))
    out = T.ToDense(5)(d)
    assert out.edge_index is None and out.edge_attr is None
    assert out.adj.shape == (5, 5) and out.adj.sum() == 4 and out.adj[2, 0] == 1 and out.adj[0, 2] == 0
    assert out.mask.dtype == torch.bool and out.mask.tolist() == [True, True, True, False, False]
    assert out.x.shape == (5, 2) and out.x[3:].abs().sum() == 0 and out.pos.shape == (5, 3)
    assert out.y.tolist() == [1, 2, 3, 0, 0]
    d = Data(x=torch.ones(3, 2), edge_index=ei, edge_attr=torch.arange(8.0).view(4, 2), y=torch.tensor([4]))
    out = T.ToDense()(d)
    assert out.adj.shape == (3, 3, 2) and out.adj[2, 2].tolist() == [6.0, 7.0] and out.y.tolist() == [4]   # a graph-level y
    assert out.x.shape == (3, 2) and repr(T.ToDense(7)) == "ToDense(num_nodes=7)" and "ToDense" in T.__all__
    with pytest.raises(AssertionError):
        T.ToDense(2)(Data(x=torch.ones(3, 2), edge_index=ei))
    data = [T.ToDense(4)(Data(x=torch.full((n, 2), float(n)), edge_index=torch.tensor([[0], [n - 1]]),
                              y=torch.tensor([n]))) for n in (2, 3, 4, 2, 3)]
    batches = list(DenseDataLoader(data, batch_size=2))
    assert [b.x.shape[0] for b in batches] == [2, 2, 1]
    b = batches[0]
    assert b.batch is None and b.x.shape == (2, 4, 2) and b.adj.shape == (2, 4, 4) and b.mask.shape == (2, 4)
    assert b.y.shape == (2, 1) and b.mask.sum(-1).tolist() == [2, 3] and b.adj[1, 0, 2] == 1


def test_to_dense_utils_on_host_tensors():
    """Host tensors take the recipe in plain torch ops, as utils.degree does; an
    unsorted batch does too."""
    from torch_geometric.utils import to_dense_adj, to_dense_batch
    for sizes in ([3, 1, 4], [0, 2, 5], [2, 0, 0, 5], [2, 5, 0, 0], [6]):
        starts = [0] + list(np.cumsum(sizes))
        n = sum(sizes)
        batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
        x = torch.randn(n, 3)
        B = int(batch.max()) + 1                                     # trailing graphs without nodes are not seen
        want, wmask = R.to_dense_batch(x, starts[:B + 1], 0.5)
        got, mask = to_dense_batch(x, batch, fill_value=0.5)
        assert torch.equal(got, want) and torch.equal(mask, wmask) and mask.dtype == torch.bool
        ei = torch.cat([torch.randint(0, s, (2, 7)) + starts[g] for g, s in enumerate(sizes) if s > 0], dim=1)
        ei = ei[:, torch.randperm(ei.shape[1])]                      # a few pairs repeat: the last one's attribute wins
        attr = torch.randn(ei.shape[1], 2)
        assert torch.equal(to_dense_adj(ei, batch), R.to_dense_adj(ei, starts[:B + 1], batch))
        assert torch.equal(to_dense_adj(ei, batch, attr), R.to_dense_adj(ei, starts[:B + 1], batch, attr))
    x = torch.randn(4, 2, requires_grad=True)
    out, mask = to_dense_batch(x)                                     # batch = None: one graph
    assert out.shape == (1, 4, 2) and bool(mask.all())
    (out * torch.arange(8.0).view(1, 4, 2)).sum().backward()
    assert torch.equal(x.grad, torch.arange(8.0).view(4, 2))
    batch = torch.tensor([1, 0, 1, 0, 1])                             # unsorted: ranks within each graph, in node order
    out, mask = to_dense_batch(torch.arange(5.0).view(5, 1), batch)
    assert out.view(2, 3).tolist() == [[1.0, 3.0, 0.0], [0.0, 2.0, 4.0]] and mask.tolist() == [[1, 1, 0], [1, 1, 1]]
    adj = to_dense_adj(torch.tensor([[0, 1, 4], [2, 3, 0]]), batch)
    assert adj.shape == (2, 3, 3) and adj.sum() == 3 and adj[1, 0, 1] == 1 and adj[0, 0, 1] == 1 and adj[1, 2, 0] == 1
    dup = to_dense_adj(torch.tensor([[0, 0, 0], [1, 1, 1]]), None, torch.tensor([1.0, 2.0, 3.0]))
    assert dup.shape == (1, 2, 2) and dup[0, 0, 1] == 3.0             # the last edge in edge order wins


def test_layers_choose_the_recipe_off_the_gpu():
    from torch_geometric import nn
    from torch_geometric.nn import DenseSAGEConv, dense_diff_pool
    from torch_geometric.nn.dense import _dense
    assert "DenseSAGEConv" in nn.__all__ and "dense_diff_pool" in nn.__all__
    t = K.diff_pool_inputs((2, 5, 3, 4, "01", "part"))
    assert not _dense.fused(t["adj"], t["x"], t["s"])                 # host tensors
    assert not _dense.pool_fused(t["x"], t["adj"], t["s"]) and not _dense.agg_fused(t["x"], t["adj"])
    assert _dense.AGG_FUSED_MAX_N == 128
    r = R.diff_pool(t["x"], t["adj"], t["s"], t["mask"])
    out, out_adj, link, ent = dense_diff_pool(t["x"].double(), t["adj"].double(), t["s"].double(), t["mask"])
    assert float((out - r["out"]).abs().max()) <= 1e-12 and float((out_adj - r["out_adj"]).abs().max()) <= 1e-12
    assert abs(float(link - r["link"])) <= 1e-12 and abs(float(ent - r["ent"])) <= 1e-12
    out2 = dense_diff_pool(t["x"][0], t["adj"][0], t["s"][0])          # 2-D inputs are one graph
    assert out2[0].shape == (1, 3, 4) and out2[1].shape == (1, 3, 3) and len(out2) == 4
    conv = DenseSAGEConv(4, 6, normalize=True).double()
    assert conv.weight.shape == (4, 6) and float(conv.weight.detach().abs().max()) <= 0.5 and repr(conv) == "DenseSAGEConv(4, 6)"
    for loop in (True, False):
        got = conv(t["x"].double(), t["adj"].double(), t["mask"], add_loop=loop).detach()
        want = R.dense_sage(t["x"], t["adj"], conv.weight.detach(), conv.bias.detach(), t["mask"], loop, True)
        assert float((got - want).abs().max()) <= 1e-12
    assert conv(t["x"][0].double(), t["adj"][0].double()).shape == (1, 5, 6)
    assert DenseSAGEConv(4, 6, bias=False).bias is None


def test_the_unit_is_registered(lib):
    import ctypes
    from mi355_mp import _lib
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "mp_dense.hip" in re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert re.search(r"^asan_dense:", mk, flags=re.M)
    assert '"asan_dense"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    names = sorted(n for n in _lib.SIGNATURES if n.startswith(("mp_diff_pool_", "mp_dense_", "mp_to_dense_")))
    assert len(names) == 10
    for name in names:
        res = _lib.SIGNATURES[name][0]
        assert res is (ctypes.c_size_t if name.endswith("_workspace") else ctypes.c_int64), name
        assert name not in _lib.STATUS_RETURNING and hasattr(lib, name)
    assert lib.mp_abi_version() == 7


def test_abi_rejections_as_a_plain_program():
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC, "asan_dense"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", HIP_VISIBLE_DEVICES="",
               ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([os.path.join(CSRC, "build", "asan", "abi_reject_dense")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.match(r"abi_reject_dense: (\d+) cases, 0 failures", r.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) >= 140, r.stdout[-500:]
    assert r.stdout.count("holds") >= 20                              # every extent and workspace, one byte short
    assert r.stdout.count("not 4-byte aligned") >= 25 and r.stdout.count("is NULL") >= 30
