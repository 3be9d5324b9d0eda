"""Writes the measured error / bar ratios of the LPIPS checks (tests/lpips_util.py: tap kernel, tap features and scalars of the whole
network) for one device into a text file: profiles/lpips_parity.txt holds the emulator's and the GPU's.
    python tools/lpips_parity.py --device cpu|cuda:0 [--cases emu|all] --out FILE     (appends a section)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--cases", default=None, choices=("emu", "all"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_parity.txt"))
    args = ap.parse_args()
    import lpips_util as LU
    cases = LU.NET_CASES
    if (args.cases or ("emu" if args.device == "cpu" else "all")) == "emu":
        import test_lpips_emu
        cases = test_lpips_emu.EMU_NET_CASES
    what = "CPU emulation build of the kernels" if args.device == "cpu" else "MI355X, product library"
    lines = [f"# {what}: measured error / bar (<= 1 passes); bars as stated in tests/lpips_util.py", "# tap kernel against fp64, bar (C + H W + 16) 2^-24 relative"]
    for c in LU.TAP_CASES:
        r = LU.check_tap(args.device, *c)
        lines.append(f"tap      N={c[0]} H={c[1]} W={c[2]} C={c[3]:<4d} worst pair {max(r):.4f}")
    lines.append("# whole network against the fp64 restatement: features 8 x the fp32 restatement's relative L2 error, scalar 8 |d32 - d64| + (512 + H W + 16) 2^-24 d64")
    worst = 0.0
    for c in cases:
        for name, ratio, a, b in LU.check_network(args.device, *c):
            worst = max(worst, ratio)
            if "feature" in name:
                lines.append(f"network  n={c[0]} {c[1]}x{c[2]:<3d} {name:<14s} {ratio:.4f}   rel-L2 {a:.3e}, fp32 restatement {b:.3e} ({a / b:.2f} x)")
            else:
                lines.append(f"network  n={c[0]} {c[1]}x{c[2]:<3d} {name:<14s} {ratio:.4f}   {a:.8e} against {b:.8e}")
    lines.append(f"# {len(cases)} network cases, largest ratio {worst:.4f}")
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
