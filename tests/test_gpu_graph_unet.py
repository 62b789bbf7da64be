"""GraphUNet: augment_adj against the dense (A + I)^2 less its diagonal; shapes, gradients, repr; the example."""
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_graph(n, e, seed, isolated=0):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n - isolated, (2, e), generator=g)
    ei = ei[:, ei[0] != ei[1]]
    key = torch.unique(ei[0] * n + ei[1])
    return torch.stack([key // n, key % n])


@pytest.mark.parametrize("n,e,isolated", [(53, 160, 0), (47, 60, 9)])
def test_augment_adj_is_the_squared_adjacency_without_its_diagonal(n, e, isolated):
    from torch_geometric.nn import GraphUNet
    ei = _random_graph(n, e, n, isolated)
    w = torch.randint(1, 4, (ei.shape[1],), generator=torch.Generator().manual_seed(1)).float()
    dev = torch.device("cuda:0")
    idx, val = GraphUNet(4, 4, 2, depth=1).augment_adj(ei.to(dev), w.to(dev), n)
    P = torch.eye(n, dtype=torch.float64).index_put_((ei[0], ei[1]), w.double())       # no loops in ei
    sq = P @ P
    mask = ((P != 0).double() @ (P != 0).double() > 0) & ~torch.eye(n, dtype=torch.bool)
    want = mask.nonzero().t()
    assert torch.equal(idx.cpu(), want)
    assert torch.equal(val.cpu(), sq[want[0], want[1]].float())


@pytest.mark.parametrize("sum_res", [True, False])
def test_graph_unet_forward_backward(sum_res):
    from torch_geometric.nn import GraphUNet
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    n = 60
    a, b = _random_graph(32, 120, 3), _random_graph(28, 100, 4) + 32
    ei = torch.cat([a, b], dim=1).to(dev)
    batch = torch.cat([torch.zeros(32, dtype=torch.int64), torch.ones(28, dtype=torch.int64)]).to(dev)
    model = GraphUNet(9, 16, 5, depth=2, pool_ratios=[0.6, 0.5], sum_res=sum_res).to(dev)
    assert repr(model) == "GraphUNet(9, 16, 5, depth=2, pool_ratios=[0.6, 0.5])"
    out = model(torch.randn(n, 9, device=dev), ei, batch)
    assert out.shape == (n, 5) and bool(torch.isfinite(out).all())
    out.square().sum().backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0, name


def test_example_trains():
    """examples/graph_unet.py --nodes 2708 --epochs 10 (10 epochs: a few seconds on an MI355X, most of
    them torch's start-up): exit 0 and a lower training loss at the end than at the start."""
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pytorch_geometric-1_amd"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "graph_unet.py"), "--nodes", "2708", "--epochs",
                        "10"], capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(x) for x in re.findall(r"loss ([0-9.]+)", r.stdout)]
    assert len(losses) == 10 and losses[-1] < losses[0], losses
