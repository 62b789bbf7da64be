"""The index arithmetic of k_agg_flat's rolling gather window, on the CPU.

csrc/mp_flat_ring.h holds what the scalar-batch loop computes with slot
indices: which batches refill the ring, how far ahead the column and weight
batches are loaded, the clamp at the end of the arrays.  tests/host/
flat_ring_twin.cpp walks tasks through those same functions the way a wave
does, over col / w arrays of exactly n_edges elements, and checks every slot
consumed against the slot it should be.  It is built here as a stand-alone
program with AddressSanitizer and UBSan, so a look-ahead that leaves the arrays
or a task is a failure, not a silent read.

Schedules: every task length that puts the task's end somewhere else in the
batch structure (1, U - 1, U, U + 1, 2U - 1, 2U, 2U + 1, 3U, 3U + 1 and a long
one), each of them once as the final task, whose look-ahead reaches n_edges;
arrays shorter than one batch; seeded random task lengths."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch_geometric-1_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "flat_ring_twin.cpp")
US = (4, 6, 8, 16)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("flat_ring") / "flat_ring_twin")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC, SRC, "-o", exe])
    return exe


def _run(exe, U, lengths, first=0, pad=0):
    """Tasks of these lengths back to back from slot `first`; the arrays end `pad` slots behind the last."""
    bounds = [first]
    for n in lengths:
        bounds.append(bounds[-1] + n)
    r = subprocess.run([exe, str(U), str(bounds[-1] + pad)] + [str(b) for b in bounds], capture_output=True, text=True,
                       env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": os.environ.get("PATH", "")})
    assert r.returncode == 0, "U=%d lengths=%r first=%d pad=%d:\n%s%s" % (U, lengths, first, pad, r.stdout, r.stderr)
    assert r.stdout.startswith("ok U=%d tasks=%d slots=%d " % (U, len(lengths), sum(lengths)))


def _edge_lengths(U):
    return [1, U - 1, U, U + 1, 2 * U - 1, 2 * U, 2 * U + 1, 3 * U, 3 * U + 1, 11 * U + 3]


@pytest.mark.parametrize("U", US)
def test_every_length_as_the_final_task(twin, U):
    ls = _edge_lengths(U)
    for i in range(len(ls)):
        _run(twin, U, ls[i + 1:] + ls[:i + 1])          # ls[i] ends exactly at n_edges
        _run(twin, U, ls[i + 1:] + ls[:i + 1], first=3)  # batches off any alignment of the arrays


@pytest.mark.parametrize("U", US)
def test_arrays_shorter_than_the_look_ahead(twin, U):
    for n in (1, 2, U - 1, U, U + 1, 2 * U - 1, 2 * U, 2 * U + 1):
        _run(twin, U, [n])               # one task is the whole array
        for pad in (1, U - 1, U, 2 * U):
            _run(twin, U, [n], pad=pad)  # the look-ahead may read on, inside the array


@pytest.mark.parametrize("U", US)
def test_random_schedules(twin, U):
    rng = random.Random(1000 + U)
    for _ in range(8):
        ls = [rng.choice((1, 2, 3, U - 1, U, U + 1, 2 * U, rng.randint(1, 5 * U))) for _ in range(rng.randint(1, 60))]
        _run(twin, U, ls, first=rng.randint(0, 5), pad=rng.choice((0, 0, 1, U)))
