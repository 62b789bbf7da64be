"""Does the compiler still emit the rolling gather window the way DESIGN 4.1 describes it?

The window of k_agg_flat's scalar-batch loop (csrc/mp_aggregate.hip) rests on
three empty asm statements that keep hipcc's schedule and its s_waitcnt
placement in shape: SumRed::pin() (the accumulate stays in front of the refill
of the ring entry it consumed), begin_at<true> (a row's initial-value load is
waited for where it is issued) and the one in row_ptr (likewise the refill of
the rowptr window).  If a compiler update moves any of them the results stay
right and only the speed goes, so nothing in the test suite would notice.
This compiles the unit for gfx950 (device only, about a minute and a half, no
GPU needed) and checks the flagship instance's code:

  * the ring's prologue issues R gathers, the steady loop R refills, and each
    refill follows an `s_waitcnt vmcnt(R - 1)` (one slot consumed, one issued)
    with no `vmcnt(0)` and no copy of a ring register in between;
  * every `v_readlane` of the rowptr window and every accumulate of the steady
    loop is reached without an `s_waitcnt vmcnt(0)` in its own basic block.

Usage: python tools/check_flat_ring_isa.py [--keep FILE.s]     exit status 0 / 1
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch_geometric-1_amd", "csrc")
KERNEL = "_ZN2mp10k_agg_flatINS_6SumRedILi1ELb1ELb0EEELi1ELi8ELi64ELb0ELb1ELi0ELb0EEEvNS_7AggArgsE"
R = 4


def function_text(path):
    out, on = [], False
    for line in open(path):
        if line.startswith(KERNEL + ":"):
            on = True
        if on:
            out.append(line.rstrip("\n"))
            if "s_endpgm" in line:
                break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default="", help="write the kernel's ISA here")
    args = ap.parse_args()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "agg.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                               "-munsafe-fp-atomics", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S",
                               os.path.join(CSRC, "mp_aggregate.hip"), "-o", asm])
        text = function_text(asm)
    if args.keep:
        with open(args.keep, "w") as f:
            f.write("\n".join(text) + "\n")
    assert text, "the flagship instance is not in the unit"
    bad = []
    gathers = [i for i, l in enumerate(text) if re.search(r"\bbuffer_load_dword\b", l)]
    if len(gathers) != 2 * R:
        bad.append("%d gathers in the code, %d expected (prologue + refills)" % (len(gathers), 2 * R))
    ring = {re.search(r"buffer_load_dword (v\d+)", text[i]).group(1) for i in gathers[:R]}
    for i in gathers[R:]:
        dst = re.search(r"buffer_load_dword (v\d+)", text[i]).group(1)
        if dst not in ring:
            bad.append("line %d: a refill lands in %s, not in a ring register %s" % (i, dst, sorted(ring)))
        j = i - 1
        while j >= 0 and not text[j].startswith(".LBB") and "s_waitcnt vmcnt" not in text[j]:
            j -= 1
        if "vmcnt(%d)" % (R - 1) not in text[j]:
            bad.append("line %d: the refill's block waits with %r, not vmcnt(%d)" % (i, text[j].strip(), R - 1))
    for i, l in enumerate(text):
        if "v_readlane_b32" in l or (gathers and gathers[R - 1] < i < gathers[-1] and "v_add_f32" in l):
            j = i - 1
            while j >= 0 and not text[j].startswith(".LBB"):
                if "vmcnt(0)" in text[j] and "v_readlane" in l and any("global_load" in t for t in text[max(0, j - 6):j]):
                    break   # the wait of a load issued in this very block, in front of its own use
                if "vmcnt(0)" in text[j]:
                    bad.append("line %d: %s sits behind an s_waitcnt vmcnt(0) of its own block" % (i, l.split()[0]))
                    break
                j -= 1
    print("flagship instance: %d lines, %d gathers, ring registers %s, %d x s_waitcnt vmcnt(0)"
          % (len(text), len(gathers), sorted(ring), sum("vmcnt(0)" in l for l in text)))
    for b in bad:
        print("FAIL " + b)
    print("ok" if not bad else "%d finding(s)" % len(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
