"""EMA of the weights (dgs_amd/ema.py, include/dgs_ema.h) against the reference's callback written with torch ops
(diffusionGS/utils/ema.py), at the shipped model size: 24 blocks, width 1024, ~460 M parameters (p, g, m, v and the shadows: ~9 GB).
Two comparisons, the two forms alternating inside one call, five pairs, every pair reported:
    step   (A) FusedAdamW.step with the EMA attached (dgs_adamw_ema_step: one launch)
           (B) FusedAdamW.step without it + the reference's `apply_ema` loop (three torch ops per tensor)
    swap   (A) `with ema.swapped(model): pass` (dgs_ema_apply in, dgs_ema_apply out: only the engine's operand copies are written)
           (B) the reference's `replace_model_weights` + `restore_original_weights` (weights to the host, load_state_dict, twice)
               followed by `model.refresh_engine_weights()`
and, alone: the plain FusedAdamW.step (what the EMA adds to the launch) and the standalone `ema.update(model)`.  Wall clock around a
synchronised loop after warm-up (form (B) of the swap waits for the host anyway).  Bytes from shapes over the best time as a share of the
measured copy bandwidth (6.29 TB/s, float4 copy on the MI355X).  Writes profiles/ema_bench.json.
    python tools/ema_bench.py [--pairs 5] [--iters 10] [--layers 24] [--out profiles/ema_bench.json]
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
import torch

from dgs_amd import denoiser as dn
from dgs_amd.ema import EMA
from dgs_amd.optim import FusedAdamW

COPY_BW = 6.29e12
DECAY = 0.9999


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3          # milliseconds per call


class ReferenceCallback:
    """The reference's EMA callback, method for method (utils/ema.py:70-76, 94-101, 152-161), without Lightning around it."""

    def __init__(self, module, decay):
        self.decay = decay
        self._ema_model_weights = [p.detach().clone() for p in module.state_dict().values()]

    def apply_ema(self, module):
        for orig_weight, ema_weight in zip(list(module.state_dict().values()), self._ema_model_weights):
            if ema_weight.data.dtype != torch.long and orig_weight.data.dtype != torch.long:
                diff = ema_weight.data - orig_weight.data
                diff.mul_(1.0 - self.decay)
                ema_weight.sub_(diff)

    def replace_model_weights(self, module):
        self._weights_buffer = [p.detach().clone().to("cpu") for p in module.state_dict().values()]
        module.load_state_dict({k: v for k, v in zip(module.state_dict().keys(), self._ema_model_weights)})

    def restore_original_weights(self, module):
        module.load_state_dict({k: v for k, v in zip(module.state_dict().keys(), self._weights_buffer)})
        del self._weights_buffer


def byte_counts(m):
    """Bytes per launch from shapes: AdamW reads p, g, m, v and writes p, m, v (28 B / parameter) and every engine copy; the EMA adds a
    read and a write of the shadow (8); the standalone update reads p and the shadow and writes the shadow (12); one direction of the
    swap reads one fp32 source (4) and writes the copies."""
    n, copies = 0, 0
    dst = m.engine().weight_destinations()
    for name, p in m.named_parameters():
        n += p.numel()
        copy, copy_t = dst.get(name, (None, None))
        copies += (0 if copy is None else copy.numel() * copy.element_size()) + (0 if copy_t is None else copy_t.numel() * 2)
    return dict(parameters=n, adamw=28 * n + copies, adamw_ema=36 * n + copies, update=12 * n, swap_one_way=4 * n + copies)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/ema_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    m = dn.DGSDenoiser(dict(width=1024, in_channels=9, patch_size=8, num_layers=a.layers, ray_pe_type="relative_plk"), device=dev)
    m.reset_parameters(seed=0)
    m = m.to(dev)
    m.engine()._train_state()                       # the training path's transposed copies exist, as in a trainer
    g = torch.Generator(device=dev).manual_seed(0)
    for p in m.parameters():
        p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
    opt = FusedAdamW(m, lr=1e-5, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.0)
    ema = EMA(m, decay=DECAY)
    ref = ReferenceCallback(m, DECAY)
    nbytes = byte_counts(m)

    def step_fused():
        opt.attach_ema(ema)
        opt.step()

    def step_plain():
        opt.attach_ema(None)
        opt.step()

    def step_reference():
        step_plain()
        ref.apply_ema(m)

    def swap_fused():
        with ema.swapped(m):
            pass

    def swap_reference():
        ref.replace_model_weights(m)
        ref.restore_original_weights(m)
        m.refresh_engine_weights()

    far = [10 ** 9]                                  # step numbers of its own: never the optimizer's next count (`step != cur_step`)

    def update():
        far[0] += 1
        ema.update(m, step=far[0])

    # the two forms compute the same shadows, bit for bit: the comparison is between equals
    check = ReferenceCallback(m, DECAY)
    step_fused()
    check.apply_ema(m)
    agree = all(torch.equal(e, w) for e, w in zip(ema.shadow_state_dict().values(), check._ema_model_weights))
    del check
    for fn in (step_fused, step_reference, swap_fused, swap_reference, update):            # warm-up: tables planned, allocator settled
        fn()
        fn()
    steps, swaps = [], []
    for _ in range(a.pairs):
        steps.append((timed(step_fused, a.iters), timed(step_reference, a.iters)))
        print(json.dumps(dict(step_ms=dict(fused=round(steps[-1][0], 3), reference=round(steps[-1][1], 3)))), flush=True)
    for _ in range(a.pairs):
        swaps.append((timed(swap_fused, a.iters), timed(swap_reference, 1)))
        print(json.dumps(dict(swap_ms=dict(fused=round(swaps[-1][0], 3), reference=round(swaps[-1][1], 3)))), flush=True)
    plain = [timed(step_plain, a.iters) for _ in range(a.pairs)]
    upd = [timed(update, a.iters) for _ in range(a.pairs)]
    share = lambda b, ms: round(b / (ms * 1e-3) / COPY_BW, 3)
    P = nbytes["parameters"]
    res = dict(device=torch.cuda.get_device_name(0), layers=a.layers, width=1024, parameters=P, decay=DECAY, copy_bandwidth=COPY_BW,
               iters_per_measurement=a.iters, fused_shadows_equal_the_reference_loop=bool(agree),
               step=dict(pairs_ms=[dict(fused=round(x, 3), adamw_then_reference_loop=round(y, 3)) for x, y in steps],
                         fused_faster_in_every_pair=all(x < y for x, y in steps), speedup_min=round(min(y / x for x, y in steps), 2),
                         bytes_per_parameter=round(nbytes["adamw_ema"] / P, 2), share_of_copy_bandwidth=share(nbytes["adamw_ema"], min(x for x, _ in steps))),
               plain_step=dict(ms=[round(x, 3) for x in plain], bytes_per_parameter=round(nbytes["adamw"] / P, 2),
                               share_of_copy_bandwidth=share(nbytes["adamw"], min(plain)),
                               ema_adds_ms=round(min(x for x, _ in steps) - min(plain), 3)),
               update=dict(ms=[round(x, 3) for x in upd], bytes_per_parameter=round(nbytes["update"] / P, 2),
                           share_of_copy_bandwidth=share(nbytes["update"], min(upd))),
               swap=dict(pairs_ms=[dict(swapped_in_and_out=round(x, 3), reference_replace_restore_refresh=round(y, 3)) for x, y in swaps],
                         fused_faster_in_every_pair=all(x < y for x, y in swaps), speedup_min=round(min(y / x for x, y in swaps), 1),
                         bytes_per_parameter_both_ways=round(2 * nbytes["swap_one_way"] / P, 2),
                         share_of_copy_bandwidth=share(2 * nbytes["swap_one_way"], min(x for x, _ in swaps))))
    res["fused_faster_in_every_pair"] = res["step"]["fused_faster_in_every_pair"] and res["swap"]["fused_faster_in_every_pair"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    print("wrote", a.out, "| (A) faster in every pair of both comparisons:", res["fused_faster_in_every_pair"])


if __name__ == "__main__":
    main()
