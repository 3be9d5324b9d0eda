"""Parity report of the mesh decimation on the device: every case of tests/test_mesh_decimate.py and tests/test_mesh_decimate_gpu.py
through the C ABI on the GPU against the numpy restatement of tests/mesh_decimate_util.py -- per case V, F, n, the five counts and
whether vertices (bit patterns), faces and counts are identical.  Writes profiles/mesh_decimate_parity.txt.
    python tools/mesh_decimate_parity.py [--out profiles/mesh_decimate_parity.txt]
Needs a GPU: there is no fallback."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mesh_decimate_util as D
from dgs_amd import _native
from test_mesh_decimate import FIXTURE_RUNS, HAND


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_decimate_parity.txt"))
    args = ap.parse_args()
    L = _native.lib()
    cases = [(name, D.level_set(name) + (n,)) for name, n in FIXTURE_RUNS + [("noise64_05", 32), ("noise64_05", 63), ("noise64_05", 64)]]
    cases += [(name, make()) for name, make in HAND.items()]
    lines = [f"{'case':22s} {'V':>8s} {'F':>8s} {'n':>5s} {'V out':>8s} {'F out':>8s} {'degen.':>8s} {'dupl.':>7s} {'invalid':>7s}  result"]
    bad = 0
    for name, (v, f, n) in cases:
        want = D.restatement(v, f, n)
        got = D.decimate_raw(L, v, f, n, "cuda:0")
        try:
            D.assert_identical(got, want)
            result = "identical"
        except AssertionError:
            result, bad = "DIFFERENT", bad + 1
        lines.append(f"{name:22s} {v.shape[0]:8d} {f.shape[0]:8d} {n:5d} " + " ".join(f"{c:{w}d}" for c, w in zip(got["counts"], (8, 8, 8, 7, 7))) + f"  {result}")
    lines.append(f"{len(cases)} cases, {bad} different")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    open(args.out, "w").write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
