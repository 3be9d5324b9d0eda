"""What the loss, clip, AdamW and sampler kernels achieve at the cases of tests/step_kernels_util.py, next to their yardsticks and bars
(tests/test_step_kernels_gpu.py).  The library is the one dgs_amd loads (DGS_AMD_LIBRARY names another build, e.g. the parent commit's).
    python tools/step_kernels_error.py            every check; the points-loss rows are printed whether they pass or not
    python tools/step_kernels_error.py --points   the points-loss rows only (what a build without the shifted sums gives)
    python tools/step_kernels_error.py --time     dgs_points_loss at B = 2, V = 4, 256 x 256: hip events, a warm-up, 7 batches of 2000 calls
    --emu: the CPU emulator build
Collected in profiles/step_kernels_parity.txt."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "open-diffusiongs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch

import step_kernels_util as U
from dgs_amd import _native

emu = "--emu" in sys.argv
if emu:
    from emu_util import emu_lib
    lib, dev, where = emu_lib(), "cpu", "CPU emulator build"
else:
    lib, dev = None, "cuda:0"
    where = torch.cuda.get_device_name(0) + ", " + os.path.basename(_native.LIB_PATH)

if "--time" in sys.argv:
    a, outs, keep = U.points_args(lib, dev, U.points_inputs(2, 4, 256, 256), True)
    L, st = U._lib(lib), U._stream(dev)
    call = lambda: L.dgs_points_loss(ctypes.byref(a), st)
    for _ in range(200):
        assert call() == 0
    torch.cuda.synchronize()
    batches = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(2000):
            call()
        e1.record()
        e1.synchronize()
        batches.append(e0.elapsed_time(e1) * 1000.0 / 2000)
    assert U._all_intact(*outs)
    print(f"dgs_points_loss B=2 V=4 256x256, gt + masks + gradient ({where}): us per call over 7 batches of 2000: "
          + " ".join(f"{b:.2f}" for b in batches) + f"   median {sorted(batches)[3]:.2f}")
    sys.exit(0)

print("loss, clip, AdamW and sampler kernels at their edges: " + where)
print("points loss: largest relative error against fp64 over the samples; bar = max(2e-4, 4 x fp32 torch)")
print(f"{'base, spread, HxW':24s} {'std of dist':>11s} {'quantity':9s} {'kernel':>10s} {'fp32 torch':>10s} {'ratio':>8s} {'bar':>10s}")
for name, std, kernel, t32 in U.measure_points_accuracy(lib, dev):
    for what, k, t in zip(("loss", "gradient"), kernel, t32):
        bar = max(U.POINTS_TOL, U.POINTS_FACTOR * t)
        print(f"{name:24s} {std:11.1e} {what:9s} {k:10.3e} {t:10.3e} {k / t:8.2f} {bar:10.3e}" + ("" if k <= bar else "   ABOVE THE BAR"))
if "--points" in sys.argv:
    sys.exit(0)

for check in (U.check_points_edges, U.check_mse, U.check_resize, U.check_sumsq, U.check_adamw, U.check_sampler_step, U.check_sampler_entry):
    try:
        check(lib, dev)
        print(f"{check.__name__}: passed")
    except AssertionError as e:
        print(f"{check.__name__}: FAILED {str(e)[:300]}")
by = {}
for section, case, name, err, yard, bar, ratio in U.RECORDS:
    by.setdefault(section, []).append((case, name, err, yard, bar, ratio))
for section in ("points loss edges", "mse", "resize", "sumsq"):
    print(f"{section}: worst error / bar")
    for case, name, err, yard, bar, ratio in by.get(section, []):
        print(f"  {case:28s} {name:22s} error {err:10.3e} bar {bar:10.3e} ratio {ratio:6.3f}")
print("adamw: per tensor and quantity, the worst error / bar over steps 1, 2, 3, 10000 x decay 0, 0.05 x clip off / above / below; "
      "bar = max(4 x torch.optim.AdamW fp32, 2^-23 max|ref|)")
print(f"  {'tensor':12s} {'q':2s} {'error':>10s} {'torch fp32':>10s} {'err/torch':>9s} {'bar':>10s} {'err/bar':>8s}")
worst = {}
for case, name, err, yard, bar, ratio in by.get("adamw", []):
    key = (case.split()[-1], name)
    if key not in worst or ratio > worst[key][3]:
        worst[key] = (err, yard, bar, ratio)
for (shape, name), (err, yard, bar, ratio) in worst.items():
    print(f"  {shape:12s} {name:2s} {err:10.3e} {yard:10.3e} {(err / yard if yard else float('inf')):9.2f} {bar:10.3e} {ratio:8.3f}")
if worst:
    print(f"adamw: worst error / bar {max(w[3] for w in worst.values()):.3f}")
