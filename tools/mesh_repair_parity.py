"""Parity report of the mesh repair: every case of tests/test_mesh_repair.py, the clustered slab, and the larger meshes the other mesh
tools use (the level sets of tests/mesh_clean_util.py, raw and through the clustering's restatement at several grids) through the C ABI
against the numpy restatement of tests/mesh_repair_util.py -- per case V, F, the ten counts, the census before and after and whether
vertices (bit patterns), faces, counts and both censuses are identical.  One section per side in profiles/mesh_repair_parity.txt; a run
replaces the section of its side and keeps the other (the CPU-emulated build of the kernels is a test build and does not travel to the
GPU host).
    python tools/mesh_repair_parity.py --side emulator|gpu [--out profiles/mesh_repair_parity.txt]
--side gpu needs a GPU: there is no fallback."""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mesh_decimate_util as D
import mesh_repair_util as R
from test_mesh_repair import CASES, SLAB_N

TITLES = {"emulator": "CPU-emulated build of csrc/mesh_repair.hip", "gpu": "MI355X, the product library"}
LARGER = (("sphere", ()), ("torus", (6,)), ("blobs", (9,)), ("noise24_05", (7, 11)), ("noise24_08", (9,)), ("noise64_08", (20,)), ("noise64_05", (26, 44)))


def clustered(name, n):
    out = D.restatement(*R.level_set(name), n)
    return out["vertices"], out["faces"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", required=True, choices=sorted(TITLES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_repair_parity.txt"))
    args = ap.parse_args()
    if args.side == "emulator":
        from emu_util import emu_lib
        L, device = emu_lib(), "cpu"
    else:
        from dgs_amd import _native
        L, device = _native.lib(), "cuda:0"
    cases = [(name, make()) for name, make in CASES.items()]
    cases.append((f"slab_clustered_{SLAB_N}", clustered_slab()))
    for name, grids in LARGER:
        cases.append((name, R.level_set(name)))
        cases += [(f"{name}_clustered_{n}", clustered(name, n)) for n in grids]
    lines = [f"== {args.side}: {TITLES[args.side]} ==",
             f"{'case':28s} {'V':>7s} {'F':>7s} | {'V_out':>7s} {'F_out':>7s} {'inval':>5s} {'null':>5s} {'dupl':>5s} {'nm e':>6s} {'remov':>6s} {'nm v':>6s} {'added':>6s} {'unref':>6s}"
             f" | nm edges, vertices before -> after | result"]
    bad = 0
    for name, (v, f) in cases:
        want = R.restatement(v, f)
        before, after = R.census(v.shape[0], f)["numbers"], R.census(want["vertices"].shape[0], want["faces"])["numbers"]
        try:
            R.assert_identical(R.repair_raw(L, v, f, device), want)
            assert R.topology_raw(L, v.shape[0], f, device) == before and R.topology_raw(L, want["vertices"].shape[0], want["faces"], device) == after
            assert after[2] == 0 and after[3] == 0
            result = "identical"
        except AssertionError:
            result, bad = "DIFFERENT", bad + 1
        lines.append(f"{name:28s} {v.shape[0]:7d} {f.shape[0]:7d} | " + " ".join(f"{c:{w}d}" for c, w in zip(want["counts"], (7, 7, 5, 5, 5, 6, 6, 6, 6, 6))) +
                     f" | {before[2]:6d} {before[3]:6d} -> {after[2]:d} {after[3]:d} | {result}")
    lines.append(f"{len(cases)} cases, {bad} different")
    section = "\n".join(lines) + "\n"
    print(section, end="")
    old = open(args.out).read() if os.path.exists(args.out) else ""
    kept = {m.group(1): m.group(0) for m in re.finditer(r"== (\w+): .*?\n(?:(?!== ).*\n)*", old)}
    kept[args.side] = section
    open(args.out, "w").write("\n".join(kept[k] for k in sorted(kept)))
    return 1 if bad else 0


def clustered_slab():
    out = D.restatement(*R.slab(), SLAB_N)
    return out["vertices"], out["faces"]


if __name__ == "__main__":
    sys.exit(main())
