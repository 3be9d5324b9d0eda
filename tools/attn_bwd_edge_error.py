"""What the attention backward achieves at the edge cases of tests/attn_bwd_util.py against fp64 autograd, next to the fp64 restatement
of its five bf16 roundings (the yardstick of tests/test_attention_backward_edges_gpu.py: kernel <= 3 x model): per case and granularity
((tensor, sample, head) slice, 64-row tile, row, tail-token rows) the worst normalised RMS error of the model, of the kernel, and their
ratio.  The launches go through the guarded call of the tests.  --emu: the CPU emulator build (cases with L <= 1026).
    python tools/attn_bwd_edge_error.py > attn_bwd_edges_parity.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "open-diffusiongs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch

import attn_bwd_util as U
from dgs_amd.dit import DitOps

emu = "--emu" in sys.argv
if emu:
    from emu_util import emu_lib
    ops, dev, before = DitOps(lib=emu_lib()), "cpu", None
else:
    ops, dev = DitOps(), "cuda:0"
    before = ops.poison_lds
print("attention backward at sequence-length and batch edges: " + ("CPU emulator build" if emu else torch.cuda.get_device_name(0)))
print(f"{'case':22s} {'granularity':11s} {'model':>10s} {'kernel':>10s} {'ratio':>6s}")
top = 0.0
for case, outliers in [(c, False) for c in U.CASES if not emu or c[0] <= U.EMU_MAX_L] + [(U.OUTLIER_CASE, True)]:
    data = U.case_data(case, outliers, dev)
    inp = data["inp"]
    o, lse2 = U.run_forward(ops, data, check=False, before_launch=before, quiet=True)
    got = U.guarded_call(ops, inp, o, lse2, before_launch=before)["dqkv"].reshape(inp["B"], inp["lpad"], 3 * inp["W"])[:, :inp["L"]]
    kw, mw = U.worst(U.errors(got, data["dref"])), U.worst(data["model_err"])
    name = U.case_id(case) + (" outliers" if outliers else "")
    for gran in ("slice", "tile", "row", "tail"):
        if gran == "tail" and not U.blocks(inp["L"])[1]:
            continue
        ratio = kw[gran] / mw[gran]
        if not outliers and gran != "tail":
            top = max(top, ratio)
        print(f"{name:22s} {gran:11s} {mw[gran]:10.3e} {kw[gran]:10.3e} {ratio:6.2f}", flush=True)
print(f"worst ratio over the asserted granularities (slice, tile, row; without the outlier case): {top:.2f}")
