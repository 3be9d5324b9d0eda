"""A/B of two builds of the library on the attention kernel: bit-compare of the outputs (the two builds are expected to execute
the same arithmetic) at the production and the tail-shaped lengths, then alternating timed launches (HIP events).
    python tools/attn_ab.py <base.so> [<new.so>]        (new defaults to the product library)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
import torch

from dgs_amd import _native
from dgs_amd.dit import DitOps

DEV = "cuda:0"
base = DitOps(_native.open_library(os.path.abspath(sys.argv[1])))
new = DitOps(_native.open_library(os.path.abspath(sys.argv[2])) if len(sys.argv) > 2 else None)
heads, W = 16, 1024
g = torch.Generator(device=DEV).manual_seed(0)
bf = lambda *s: torch.randn(*s, generator=g, device=DEV).to(torch.bfloat16)


def case(L, B):
    lpad = (L + 255) // 256 * 256
    qk, vt = bf(B * lpad, 2 * W), bf(B, W, lpad)
    qk[3, :64] *= 6.0              # a spiky query row and key row: the rescale branch
    qk[70 % L, W:W + 64] *= 6.0
    return qk, vt, lpad


for L, B in ((4098, 1), (4130, 1), (290, 2), (18, 2), (1026, 1), (600, 1), (16386, 1)):
    qk, vt, lpad = case(L, B)
    la, lb = torch.zeros(B, heads, lpad, device=DEV), torch.zeros(B, heads, lpad, device=DEV)
    for ops in (base, new):
        ops.poison_lds()
    a = base.attention(qk, vt, L, heads, lse2=la, q_prescaled=True)
    b = new.attention(qk, vt, L, heads, lse2=lb, q_prescaled=True)
    torch.cuda.synchronize()
    va, vb = a.view(B, lpad, W)[:, :L], b.view(B, lpad, W)[:, :L]
    same = torch.equal(va.view(torch.int16), vb.view(torch.int16)) and torch.equal(la[:, :, :L], lb[:, :, :L])
    nm = L // 32 * 32                                   # rows of the main path; the L % 32 tail queries are merged from per-tile records
    main_same = torch.equal(va[:, :nm].contiguous().view(torch.int16), vb[:, :nm].contiguous().view(torch.int16)) and torch.equal(la[:, :, :nm], lb[:, :, :nm])
    tail = f"; main rows bit-identical: {main_same}, tail rows max |diff| {float((va[:, nm:].float() - vb[:, nm:].float()).abs().max()):.3g}" if nm < L else ""
    print(f"L={L} B={B}: outputs bit-identical: {same}; finite: {bool(torch.isfinite(vb.float()).all())}; "
          f"max |diff| {float((va.float() - vb.float()).abs().max()):.3g}{tail}", flush=True)

ROUNDS = 7
for L, B, n in ((4098, 1, 40), (4098, 4, 12), (16386, 1, 6)):
    # per round: n alternating launches of base, base again and new; a new / base ratio means something only against the spread of the
    # base / base ratios of the same run
    qk, vt, lpad = case(L, B)
    runs = (("base", base), ("base2", base), ("new", new))
    for _ in range(5):
        base.attention(qk, vt, L, heads, q_prescaled=True); new.attention(qk, vt, L, heads, q_prescaled=True)
    bb, nb, med = [], [], {}
    for _ in range(ROUNDS):
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)] for k, _ in runs}
        for i in range(n):
            for k, ops in runs:
                e0, e1 = ev[k][i]
                e0.record(); ops.attention(qk, vt, L, heads, q_prescaled=True); e1.record()
        torch.cuda.synchronize()
        med = {k: sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in v)[n // 2] for k, v in ev.items()}
        bb.append(med["base2"] / med["base"]); nb.append(med["new"] / med["base"])
    flops = 4.0 * L * L * W * B
    print(f"timing L={L} B={B}: last round base {med['base']:.1f} us ({flops / med['base'] / 1e6:.0f} TFLOP/s)  new {med['new']:.1f} us "
          f"({flops / med['new'] / 1e6:.0f} TFLOP/s)  (median of {n}, incl. the output memset)\n"
          f"    base / base per round " + " ".join(f"{r:.3f}" for r in bb) + "\n    new  / base per round " + " ".join(f"{r:.3f}" for r in nb) +
          f"\n    new / base median {sorted(nb)[ROUNDS // 2]:.3f}; base / base spread [{min(bb):.3f}, {max(bb):.3f}]: "
          f"{'all below' if max(nb) < min(bb) else 'all above' if min(nb) > max(bb) else 'overlaps'}", flush=True)
