"""What the DiT row kernels achieve against fp64 at the cases of tests/rowkernel_util.py, next to the derived bars of
tests/test_dit_rowkernels_gpu.py: per kernel, case and output the worst error / bar over the case's forms, the error and the bar at that
element, and for bf16 outputs the share of elements that took the either-neighbour exception at a rounding midpoint (cap 0.5 %).
The launches go through the guarded calls of the tests.  --emu: the CPU emulator build at the emulator test's cases.
    python tools/dit_rowkernel_error.py > profiles/dit_rowkernels_parity.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "open-diffusiongs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch

import rowkernel_util as R
from dgs_amd.dit import DitOps

emu = "--emu" in sys.argv
if emu:
    from emu_util import emu_lib
    lib, dev, before = emu_lib(), "cpu", None
    R.check_layernorm(lib, dev, widths=(256, 1024), shapes=R.LN_SHAPES[:1])
    R.check_rowlinear(lib, dev, Ms=(1, 3, 16), Ns=(14, 37), Ks=(256, 512, 1024))
    R.check_layernorm_backward(lib, dev, widths=(256, 1024), Bs=(1, 3), rpbs=(5, 24), masks=(1, 6, 7))
    R.check_rowlinear_backward(lib, dev, shapes=[(3, 70, 256), (8, 257, 1024)], per_shape=9)
    R.check_gate_mul(lib, dev, cases=[(3, 64, 64)])
else:
    ops, dev = DitOps(), "cuda:0"
    lib, before = ops.lib, ops.poison_lds
    R.check_layernorm(lib, dev, before=before)
    R.check_rowlinear(lib, dev, before=before)
    R.check_layernorm_backward(lib, dev, before=before)
    R.check_layernorm_backward_training_partition(lib, dev, before=before)
    R.check_rowlinear_backward(lib, dev, before=before)
    R.check_gate_mul(lib, dev, before=before)

groups = {}
for kernel, case, name, err, bar, ratio, share in R.RECORDS:
    groups.setdefault((kernel, case, name), []).append((ratio, err, bar, share))
worst = {}
for k, recs in groups.items():
    ratio, err, bar, _ = max(recs, key=lambda r: r[0])
    shares = [r[3] for r in recs if r[3] is not None]
    worst[k] = (err, bar, ratio, max(shares) if shares else None, len(recs))
print("DiT row kernels against fp64: " + ("CPU emulator build" if emu else torch.cuda.get_device_name(0)))
print("error, bar: at the element with the worst error / bar over the case's forms; bf16 outputs: bar = half a bf16 step + the fp32 bound")
print(f"{'kernel':19s} {'case':34s} {'output':9s} {'forms':>5s} {'error':>10s} {'bar':>10s} {'ratio':>6s} {'exception share':>15s}")
top, top_share = {}, 0.0
for (kernel, case, name), (err, bar, ratio, share, count) in worst.items():
    top[kernel] = max(top.get(kernel, 0.0), ratio)
    top_share = max(top_share, share or 0.0)
    print(f"{kernel:19s} {case:34s} {name:9s} {count:5d} {err:10.3e} {bar:10.3e} {ratio:6.3f} " + (f"{100 * share:14.4f}%" if share is not None else ""))
# which term of the bound a ratio above 0.5 sits on (the bounds themselves: tests/rowkernel_util.py)
TERM = {("layernorm", "out f32"): "the output's own last operations -- u |n| of c rstd, u |n w|, 2 u |t| of (1 + scale) and its product, u |y| of the "
                                  "final add: 2 - 5 roundings on rows whose statistics contribute little, of which a correct kernel spends 1 - 3",
        ("rowlinear_backward", "dW"): "(MR + 1) u sum|terms|: the product's rounding and MR <= 8 additions, 2 - 5 roundings at M <= 4",
        ("rowlinear_backward", "db"): "MR u sum|dy|: a chain of MR <= 8 additions, 2 - 4 roundings at M <= 4"}
over = {}
for (kernel, case, name), (err, bar, ratio, share, count) in worst.items():
    if share is None and ratio > 0.5:
        over.setdefault((kernel, name), []).append(ratio)
print("bf16 outputs: half a bf16 step is the output's own rounding, so error / bar reaches 1.000 wherever a reference sits on a midpoint")
for (kernel, name), ratios in over.items():
    print(f"above 0.5: {kernel} {name}, {len(ratios)} cases, at most {max(ratios):.3f}: " + TERM.get((kernel, name), "NOT ATTRIBUTED"))
for kernel, ratio in top.items():
    print(f"worst error / bar, {kernel}: {ratio:.3f}")
print(f"worst share of bf16 elements that took the either-neighbour exception: {100 * top_share:.4f}% (cap {100 * R.EXCEPTION_CAP:.1f}%)")
