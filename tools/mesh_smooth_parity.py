"""Parity report of the mesh smoothing: every case of tests/test_mesh_smooth.py and tests/test_mesh_smooth_gpu.py through the C ABI
against the numpy restatement of tests/mesh_smooth_util.py -- per case V, F, the arguments, the four counts and whether the vertices
(bit patterns) and the counts are identical.  One section per side in profiles/mesh_smooth_parity.txt; a run replaces the section of
its side and keeps the other (the CPU-emulated build of the kernels is a test build and does not travel to the GPU host).
    python tools/mesh_smooth_parity.py --side emulator|gpu [--out profiles/mesh_smooth_parity.txt]
--side gpu needs a GPU: there is no fallback."""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mesh_smooth_util as S
from test_mesh_smooth import CASES

TITLES = {"emulator": "CPU-emulated build of csrc/mesh_smooth.hip", "gpu": "MI355X, the product library"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", required=True, choices=sorted(TITLES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_smooth_parity.txt"))
    args = ap.parse_args()
    if args.side == "emulator":
        from emu_util import emu_lib
        L, device = emu_lib(), "cpu"
    else:
        from dgs_amd import _native
        L, device = _native.lib(), "cuda:0"
    cases = [(name, make()) for name, make in CASES.items()]
    cases.append(("noise64_05", S.level_set("noise64_05") + (dict(iterations=2),)))
    lines = [f"== {args.side}: {TITLES[args.side]} ==",
             f"{'case':24s} {'V':>8s} {'F':>8s} {'it.':>4s} {'lambda':>7s} {'mu':>6s} {'fixed':>5s} {'invalid':>7s} {'null':>5s} {'over':>5s} {'unref.':>6s}  result"]
    bad = 0
    for name, (v, f, kw) in cases:
        want = S.restatement(v, f, **kw)
        try:
            S.assert_identical(S.smooth_raw(L, v, f, device, **kw), want)
            result = "identical"
        except AssertionError:
            result, bad = "DIFFERENT", bad + 1
        lines.append(f"{name:24s} {v.shape[0]:8d} {f.shape[0]:8d} {kw.get('iterations', 10):4d} {kw.get('lam', 0.5):7.2f} {kw.get('mu', -0.53):6.2f} "
                     f"{'half' if 'fixed' in kw else 'none':>5s} " + " ".join(f"{c:{w}d}" for c, w in zip(want["counts"], (7, 5, 5, 6))) + f"  {result}")
    lines.append(f"{len(cases)} cases, {bad} different")
    section = "\n".join(lines) + "\n"
    print(section, end="")
    old = open(args.out).read() if os.path.exists(args.out) else ""
    kept = {m.group(1): m.group(0) for m in re.finditer(r"== (\w+): .*?\n(?:(?!== ).*\n)*", old)}
    kept[args.side] = section
    open(args.out, "w").write("\n".join(kept[k] for k in sorted(kept)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
