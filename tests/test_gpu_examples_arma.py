"""examples/arma.py runs end to end as a program of its own and learns: every
loss is finite and the last quarter's mean is below the first quarter's."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_arma():
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pytorch_geometric-1_amd"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "arma.py"), "--epochs", "20"],
                       capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    losses = [float(v) for v in re.findall(r"^Epoch: \d+, loss ([0-9.eE+-]+|nan|inf),", r.stdout, flags=re.M)]
    assert len(losses) == 20 and all(math.isfinite(v) for v in losses), losses
    first, last = sum(losses[:5]) / 5, sum(losses[-5:]) / 5
    print("arma: loss %.4f over the first 5 epochs, %.4f over the last" % (first, last))
    assert last < first, (first, last)
