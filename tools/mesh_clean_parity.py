"""Parity report of the mesh clean-up on the device: every case of tests/test_mesh_clean.py and tests/test_mesh_clean_gpu.py through the
C ABI on the GPU against the numpy restatement of tests/mesh_clean_util.py -- per case V, F, min_f, min_d, the five counts and whether
vertices (bit patterns), faces, labels and counts are identical.  Writes profiles/mesh_clean_parity.txt.
    python tools/mesh_clean_parity.py [--out profiles/mesh_clean_parity.txt]
Needs a GPU: there is no fallback."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mesh_clean_util as C
from dgs_amd import _native
from test_mesh_clean import FIXTURE_RUNS, HAND


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_clean_parity.txt"))
    args = ap.parse_args()
    L = _native.lib()
    cases = [(f"{name}", C.level_set(name) + (min_f, min_d), C.level_set_components(name)) for name, min_f, min_d in FIXTURE_RUNS]
    cases += [(name, C.level_set(name) + (min_f, min_d), C.level_set_components(name))
              for name, min_f, min_d in (("noise64_05", 64, 20.0), ("noise64_08", 64, 20.0), ("noise64_08", 64, 0.0))]
    cases += [(name, make(), None) for name, make in HAND.items()]
    lines = [f"{'case':28s} {'V':>8s} {'F':>8s} {'min_f':>5s} {'min_d':>5s} {'V kept':>8s} {'F kept':>8s} {'comps':>6s} {'kept':>5s} {'invalid':>7s}  result"]
    bad = 0
    for name, (v, f, min_f, min_d), comp in cases:
        want = C.restatement(v, f, min_f, min_d, comp)
        got = C.clean_raw(L, v, f, min_f, min_d, "cuda:0")
        try:
            C.assert_identical(got, want)
            result = "identical"
        except AssertionError:
            result, bad = "DIFFERENT", bad + 1
        lines.append(f"{name:28s} {v.shape[0]:8d} {f.shape[0]:8d} {min_f:5d} {min_d:5.1f} " + " ".join(f"{c:{w}d}" for c, w in zip(got["counts"], (8, 8, 6, 5, 7))) + f"  {result}")
    lines.append(f"{len(cases)} cases, {bad} different")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    open(args.out, "w").write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
