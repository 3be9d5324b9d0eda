"""What the DiT GEMM kernels achieve against fp64 at the cases of tests/gemm_util.py: per case and output the plan the call ran
(dgs_dit_gemm_plan), the worst 32-row block and 64-column strip, the error and the bar at that element, their ratio, and for the bf16
outputs with an error zone the share of elements that took the either-neighbour exception (cap 0.5 %).  Exact-regime outputs that are
compared bit for bit have error 0 and no bar.  The launches go through the guarded calls of the tests; a case that fails its check is
listed with the assertion's text and the run goes on.  --emu: the CPU emulator build at the emulator test's cases.
    python tools/dit_gemm_error.py > profiles/dit_gemm_parity.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "open-diffusiongs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch

import gemm_util as G

emu = "--emu" in sys.argv
if emu:
    from emu_util import emu_lib
    lib, dev, before, cases = emu_lib(), "cpu", None, G.EMU_CASES
else:
    from dgs_amd.dit import DitOps
    ops, dev, cases = DitOps(), "cuda:0", G.GPU_CASES
    lib, before = ops.lib, ops.poison_lds
failed = []
for c in cases:
    if emu:
        os.environ["DGS_EMU_CUS"] = str(c["cus"] or 6)
    try:
        G.run_case(lib, dev, c, before=before)
    except AssertionError as e:
        failed.append((c["name"], str(e)))
print("DiT GEMM kernels against fp64: " + ("CPU emulator build" if emu else torch.cuda.get_device_name(0)))
print("exact regime: bit-equal outputs have error 0 and no bar; zone outputs: bar = the activation's fp32 error zone at the worst element, ratio = error /")
print("(half a bf16 step + zone); general regime: bar = K 2^-23 sum|a w| (+ half a bf16 step for bf16 outputs), ratio = error / bar")
print(f"{'case':58s} {'regime':7s} {'output':16s} {'block':>5s} {'strip':>5s} {'error':>10s} {'bar':>10s} {'ratio':>7s} {'exceptions':>10s}  plan")
top_general, top_share = {"f32": 0.0, "bf16": 0.0}, 0.0
for name, regime, output, plan, blk, strip, err, bar, ratio, share in G.RECORDS:
    if regime == "general":
        kind = output.split()[-1]
        top_general[kind] = max(top_general[kind], ratio)
    top_share = max(top_share, share or 0.0)
    print(f"{name:58s} {regime:7s} {output:16s} {blk:5d} {strip:5d} {err:10.3e} {bar:10.3e} {ratio:7.4f} " + (f"{100 * share:9.4f}%" if share is not None else " " * 10) + "  " + plan)
print(f"cases: {len(cases)}, failed: {len(failed)}")
for name, text in failed:
    print(f"FAILED {name}: {text[:600]}")
print(f"worst error / bar in the general regime, f32 outputs: {top_general['f32']:.4f}")
print(f"worst error / (half a bf16 step + bar) in the general regime, bf16 outputs: {top_general['bf16']:.4f} -- half a step is the output's own rounding, so this")
print("reaches 1 wherever a reference sits on a rounding midpoint; the fp32 part of the bar is what the f32 line measures")
print(f"worst share of bf16 elements that took the either-neighbour exception: {100 * top_share:.4f}% (cap {100 * G.EXCEPTION_CAP:.1f}%)")
