"""examples/qm9_nn_conv.py (the reference's MPNN with its Set2Set readout, on
synthetic QM9-shaped molecules) runs end to end as a program of its own and
learns: the loss is finite and lower over the last tenth of the epoch's batches
than over the first."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_qm9_nn_conv():
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pytorch_geometric-1_amd"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "qm9_nn_conv.py"), "--epochs", "1", "--graphs", "2560"],
                       capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    losses = [float(v) for v in re.findall(r"^loss ([0-9.eE+-]+|nan|inf)$", r.stdout, flags=re.M)]
    assert len(losses) == 20 and all(math.isfinite(v) for v in losses), losses
    tenth = len(losses) // 10
    first, last = sum(losses[:tenth]) / tenth, sum(losses[-tenth:]) / tenth
    print("qm9_nn_conv: loss %.4f over the first %d batches, %.4f over the last" % (first, tenth, last))
    assert last < first, (first, last)
    assert re.search(r"^Epoch: 01, loss", r.stdout, flags=re.M)
