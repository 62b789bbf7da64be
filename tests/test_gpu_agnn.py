"""The fused AGNNConv path (csrc/mp_agnn.hip) on the GPU against float64 autograd through
oracle.pyg_ref.agnn_conv.  The graph: 300 nodes, about 4000 edges in random order with duplicates and
self loops, node 7 with 700 in-edges (split over tasks at chunk 64, finished in the fix-up), nodes 250..
without in-edges, nodes 280.. isolated, node 11 with an all-zero feature row (the 1e-12 clamp).
Bounds (those of tests/test_gpu_fuzz_layers.py for this layer): values within 1e-5 * max(1, |ref|),
gradients within 1e-4 * max(1, |ref|) + 4 * max|the formula in fp32 torch - float64|."""
import functools
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from oracle import pyg_ref as P
from tests._recurrent_lane_cases import AGNN_WIDTHS, agnn_mapping

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 300
# 1 and 3; the example's width; no multiple of 4; the last width of one vec4 per lane and the first beyond; the largest;
# then (tests/_recurrent_lane_cases.py) three vec4 per lane, 4 and 16 scalars per lane, groups of 2, 8 and 16 lanes
WIDTHS = list(AGNN_WIDTHS)
assert WIDTHS[:7] == [1, 3, 16, 18, 256, 260, 1024]


@functools.lru_cache(maxsize=None)
def _edges():
    g = torch.Generator().manual_seed(4)
    ei = torch.stack([torch.randint(0, 280, (3200,), generator=g), torch.randint(0, 250, (3200,), generator=g)])
    hub = torch.stack([torch.randint(0, 280, (700,), generator=g), torch.full((700,), 7, dtype=torch.int64)])
    loops = torch.arange(0, 60, 2).repeat(2, 1)
    ei = torch.cat([ei, ei[:, :70], hub, loops], dim=1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)].contiguous()
    assert int(torch.bincount(ei[1], minlength=N)[7]) >= 700 and int(ei[1].max()) < 250 and int(ei.max()) < 280
    return ei


@functools.lru_cache(maxsize=None)
def _case(F, beta, reverse=False):
    """Inputs and the reference's answers (float64, and the same formula in fp32) for one case, computed once."""
    ei = _edges().flip(0).contiguous() if reverse else _edges()
    g = torch.Generator().manual_seed(F)
    x = torch.randn(N, F, generator=g)
    x[11] = 0.0
    gout = torch.randn(N, F, generator=g)
    res = {}
    for dt in (torch.float64, torch.float32):
        xx, bb = x.clone().to(dt).requires_grad_(), torch.tensor([beta], dtype=dt).requires_grad_()
        out = P.agnn_conv(xx, ei, bb)
        (out * gout.to(dt)).sum().backward()
        res[dt] = (out.detach().double(), xx.grad.double(), bb.grad.double())
    return dict(x=x, ei=ei, gout=gout, ref=res[torch.float64], f32=res[torch.float32])


def _check(got, c):
    for k, (what, tol) in enumerate((("out", 1e-5), ("dx", 1e-4), ("dbeta", 1e-4))):
        want, own = c["ref"][k], 0.0 if k == 0 else float((c["f32"][k] - c["ref"][k]).abs().max())
        err = (got[k].detach().cpu().double() - want).abs()
        lim = tol * want.abs().clamp(min=1.0) + 4 * own
        print("%s: max err %.3g, fp32 formula's own %.3g, max err / bound %.3g"
              % (what, float(err.max()), own, float((err / lim).max())))
        assert bool((err <= lim).all()), (what, float(err.max()), own)


def _run(graph, x, beta):
    from mi355_mp import ops
    xd, bd = x.to(DEV).requires_grad_(), torch.tensor([beta], device=DEV, requires_grad=True)
    return xd, bd, ops.agnn_propagate(graph, xd, bd)


def _graph(c, schedule):
    from mi355_mp import ops
    from mi355_mp.graph import Graph
    from torch_geometric.nn.conv._structure import gat_loops
    ei = gat_loops(c["ei"].to(DEV), N)
    graph = Graph(ei, N, N, chunk=None if schedule == "rows" else ops.agnn_split_chunk())
    split = graph.src if schedule == "split_src" else graph.dst
    assert split.chunk < 64 if schedule == "rows" else (split.chunk == 64 and split.n_split >= 1)
    return graph


@pytest.mark.parametrize("schedule", ["rows", "split_dst", "split_src"])
@pytest.mark.parametrize("F,beta", [(f, 0.8) for f in WIDTHS] + [(16, -2.0), (16, 30.0)])
def test_kernels_against_float64(F, beta, schedule):
    c = _case(F, beta, schedule == "split_src")
    print("F = %d: (W, NV, lanes per group) = %s, %s" % (F, agnn_mapping(F), schedule))
    xd, bd, out = _run(_graph(c, schedule), c["x"], beta)
    out.backward(c["gout"].to(DEV))
    _check((out, xd.grad, bd.grad), c)


def test_two_runs_are_bitwise_equal():
    c = _case(260, 0.8)
    graph = _graph(c, "split_dst")
    runs = []
    for _ in range(2):
        xd, bd, out = _run(graph, c["x"], 0.8)
        out.backward(c["gout"].to(DEV))
        runs.append((out.detach(), xd.grad, bd.grad))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("kind,fused", [("fp32", 1), ("beta_buffer", 1), ("target_to_source", 1), ("float64", 0),
                                        ("own_message", 0), ("too_wide", 0)])
def test_layer_dispatch(kind, fused, monkeypatch):
    from mi355_mp import ops
    from torch_geometric.nn import AGNNConv

    class Own(AGNNConv):
        def message(self, edge_index_i, x_j, x_norm_i, x_norm_j, num_nodes):
            return super(Own, self).message(edge_index_i, x_j, x_norm_i, x_norm_j, num_nodes)

    calls = []
    real = ops.agnn_propagate
    monkeypatch.setattr(ops, "agnn_propagate", lambda *a: calls.append(1) or real(*a))
    flow = "target_to_source" if kind == "target_to_source" else "source_to_target"
    c = _case(1025 if kind == "too_wide" else 16, 0.8 if kind != "beta_buffer" else 1.0, flow == "target_to_source")
    dt = torch.float64 if kind == "float64" else torch.float32
    conv = (Own if kind == "own_message" else AGNNConv)(requires_grad=kind != "beta_buffer", flow=flow).to(DEV).to(dt)
    if kind != "beta_buffer":
        with torch.no_grad():
            conv.beta.fill_(0.8)
    xd = c["x"].to(DEV).to(dt).requires_grad_()
    ei = (c["ei"].flip(0) if flow == "target_to_source" else c["ei"]).to(DEV)   # the layer's view of the same graph
    out = conv(xd, ei)
    out.backward(c["gout"].to(DEV).to(dt))
    assert len(calls) == fused
    _check((out, xd.grad, conv.beta.grad if kind != "beta_buffer" else c["ref"][2]), c)
    if fused:
        del calls[:]
        with torch.no_grad():
            conv(xd, ei)
        assert len(calls) == 1 and sorted(conv.state_dict()) == ["beta"] and repr(conv) == "AGNNConv()"


def test_no_edge_feature_array():
    """Forward + backward at F = 256 peaks below ONE [E, F] fp32 array of the looped edge list."""
    from mi355_mp import _lib, ops
    from mi355_mp.graph import Graph
    F = 256
    g = torch.Generator().manual_seed(9)
    ei = torch.randint(0, N, (2, 40000), generator=g).to(DEV)
    ei = torch.cat([ei[:, ei[0] != ei[1]], torch.arange(N, device=DEV).repeat(2, 1)], dim=1).contiguous()
    graph = Graph(ei, N, N, chunk=ops.agnn_split_chunk())
    E = ei.shape[1]
    slabs = sum(_lib.native().mp_agnn_workspace(csr.struct("other"), F, k)
                for csr, k in ((graph.dst, 0), (graph.dst, 1), (graph.src, 2)))
    own = 5 * N * F * 4 + 2 * E * 4 + slabs              # x, out, g, dx, u; alpha, bds; the three workspaces
    one = E * F * 4
    assert 2 * own < one, (own, one)
    x = torch.randn(N, F, generator=g).to(DEV).requires_grad_()
    beta = torch.ones(1, device=DEV, requires_grad=True)
    gout = torch.randn(N, F, generator=g).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ops.agnn_propagate(graph, x, beta).backward(gout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak %d bytes, one [E, F] array %d" % (peak, one))
    assert peak < one


def test_example_agnn():
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pytorch_geometric-1_amd"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "agnn.py"), "--epochs", "15"],
                       capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    losses = [float(v) for v in re.findall(r"^Epoch: \d+, loss ([0-9.eE+-]+|nan|inf),", r.stdout, flags=re.M)]
    assert len(losses) == 15 and all(math.isfinite(v) for v in losses), losses
    assert sum(losses[-3:]) / 3 < sum(losses[:3]) / 3, losses
