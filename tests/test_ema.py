"""EMA of the weights (include/dgs_ema.h, dgs_amd/ema.py): the shadows kept inside the AdamW launch, the table-driven launch, the swap
of the engine's operand copies for evaluation, the reference's checkpoint pair and the trainer option -- against the reference's own
expression (diffusionGS/utils/ema.py:94-101: diff = ema - w; diff.mul_(1 - decay); ema.sub_(diff)) in torch, BIT FOR BIT.  CPU-emulated
kernels here, the same comparisons on MI355X under `-m gpu` (only there can an FMA contraction of the expression show)."""
import ctypes
import os
import re
import subprocess
import tempfile
import warnings

import pytest
import torch

from dgs_amd import _native
from dgs_amd import denoiser as dn
from dgs_amd.ema import EMA
from dgs_amd.optim import FusedAdamW, flat_offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CFG = dict(width=256, in_channels=9, patch_size=8, num_layers=2)
GPU_CFG = dict(width=1024, in_channels=9, patch_size=8, num_layers=2)


def _where(gpu):
    if gpu:
        return torch.device("cuda:0"), None, GPU_CFG
    from emu_util import emu_lib
    return torch.device("cpu"), emu_lib(), CFG


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None


def ref_apply(shadows, weights, decay):
    """utils/ema.py:94-101, as it stands there."""
    for orig_weight, ema_weight in zip(weights, shadows):
        diff = ema_weight.data - orig_weight.data
        diff.mul_(1.0 - decay)
        ema_weight.sub_(diff)


def _model(dev, lib, cfg, seed=2):
    m = dn.DGSDenoiser(cfg, device=dev, lib=lib)
    m.reset_parameters(seed=seed)
    m = m.to(dev)
    m.engine()._train_state()                            # the transposed weight copies of the training path exist
    return m


def _set_grads(m, gen, scale, dev):
    """Random gradients (same tensors every step, like the trainer's flat-buffer views); returns their sum of squares, device float[1]."""
    total = torch.zeros(1, dtype=torch.float64)
    for p in m.parameters():
        gr = torch.randn(p.shape, generator=gen) * scale
        total += gr.double().pow(2).sum()
        if p.grad is None:
            p.grad = gr.to(dev)
        else:
            p.grad.copy_(gr)
    return total.float().to(dev)


def _copies_follow(m, source, tag=""):
    """Every engine copy = the bf16 / fp32 rounding of `source[key]`, transposed copies = the transposes of the bf16 ones."""
    dst = m.engine().weight_destinations()
    assert any(t is not None for _, t in dst.values())
    for n, (copy, copy_t) in dst.items():
        assert torch.equal(copy.reshape(source[n].shape), source[n].detach().to(copy.dtype)), (tag, n)
        if copy_t is not None:
            assert torch.equal(copy_t, copy.t()), (tag, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. table level
# ---------------------------------------------------------------------------------------------------------------------------------
# (rows, cols, copy dtype or None, transposed copy): numel 1, 3 and 14 take the scalar tail, 4097 takes it over two tiles, 8200 is two
# float4 tiles, the matrices go through the 64 x 64 block path (one block, and 2 x 3 blocks)
SHAPES = [(1, 1, None, False), (1, 3, torch.float32, False), (1, 14, torch.bfloat16, False), (1, 4097, torch.bfloat16, False),
          (1, 8200, torch.float32, False), (64, 64, torch.bfloat16, True), (128, 192, torch.bfloat16, True)]
DECAY = 0.9


def _device_table(host, dev):
    return torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)


def _table_case(dev, lib):
    g = torch.Generator().manual_seed(0)
    offs, total = flat_offsets(r * c for r, c, _, _ in SHAPES)
    shadow = torch.full((total,), 7.0, device=dev)                  # 7.0: the padding between slices must stay as it is
    P, E, C, CT = [], [], [], []
    for (r, c, kind, tr), off in zip(SHAPES, offs):
        P.append(torch.randn(r, c, generator=g).to(dev))
        E.append(shadow[off:off + r * c].view(r, c))
        E[-1].copy_(torch.randn(r, c, generator=g))
        C.append(None if kind is None else torch.zeros(r, c, dtype=kind, device=dev))
        CT.append(torch.zeros(c, r, dtype=torch.bfloat16, device=dev) if tr else None)
    return g, offs, total, shadow, P, E, C, CT


def _ema_table(lib, dev, P, E, C, CT, copies=True):
    entries = []
    for (r, c, kind, tr), p, e, cp, ct in zip(SHAPES, P, E, C, CT):
        t = _native.DgsEmaTensor()
        t.p, t.ema, t.rows, t.cols = p.data_ptr(), e.data_ptr(), r, c
        if copies and cp is not None:
            t.copy, t.copy_kind = cp.data_ptr(), _native.OPTIM_COPY_BF16 if kind == torch.bfloat16 else _native.OPTIM_COPY_F32
        if copies and ct is not None:
            t.copy_t = ct.data_ptr()
        entries.append(t)
    host = (_native.DgsEmaTensor * len(entries))(*entries)
    n_tiles = lib.dgs_ema_plan(host, len(entries))
    want = sum((r // 64) * (c // 64) if (tr and copies) else -(-r * c // 4096) for r, c, _, tr in SHAPES)
    assert n_tiles == want, (n_tiles, want)
    return _device_table(host, dev), len(entries), n_tiles


def _apply(lib, dev, table, update, source):
    a = _native.DgsEmaArgs()
    a.tensors, a.n_tensors, a.n_tiles = table[0].data_ptr(), table[1], table[2]
    a.one_minus_decay, a.update, a.copy_source = 1.0 - DECAY, update, source
    assert lib.dgs_ema_apply(ctypes.byref(a), _stream(dev)) == 0


def _table_level(gpu):
    dev, lib, _ = _where(gpu)
    lib = lib or _native.lib()
    g, offs, total, shadow, P, E, C, CT = _table_case(dev, lib)
    pad = torch.ones(total, dtype=torch.bool)
    for (r, c, _, _), off in zip(SHAPES, offs):
        pad[off:off + r * c] = False
    pad = pad.to(dev)

    # -- dgs_ema_apply, update only: 3 steps, the parameters moving in between --------------------------------------------
    upd = _ema_table(lib, dev, P, E, C, CT, copies=False)
    want = [e.clone() for e in E]
    for step in range(3):
        for p in P:
            p.add_(torch.randn(p.shape, generator=g).to(dev) * 0.1)
        before = [p.clone() for p in P]
        _apply(lib, dev, upd, 1, _native.EMA_SOURCE_NONE)
        ref_apply(want, P, DECAY)
        for i, (e, w, p, b) in enumerate(zip(E, want, P, before)):
            assert torch.equal(e, w), (step, SHAPES[i])
            assert torch.equal(p, b), (step, SHAPES[i])                 # p is read, never written
        assert bool((shadow[pad] == 7.0).all())
    assert all(c is None or not bool(c.any()) for c in C)               # no copies in this table: none written

    # -- copies in both modes: p and the shadows untouched ------------------------------------------------------------------
    swap = _ema_table(lib, dev, P, E, C, CT, copies=True)
    for source, src in ((_native.EMA_SOURCE_EMA, E), (_native.EMA_SOURCE_P, P)):
        keep_p, keep_e = [p.clone() for p in P], [e.clone() for e in E]
        _apply(lib, dev, swap, 0, source)
        for i, (s, cp, ct) in enumerate(zip(src, C, CT)):
            if cp is not None:
                assert torch.equal(cp, s.to(cp.dtype)), (source, SHAPES[i])
            if ct is not None:
                assert torch.equal(ct, cp.t()), (source, SHAPES[i])
        assert all(torch.equal(a, b) for a, b in zip(P, keep_p)) and all(torch.equal(a, b) for a, b in zip(E, keep_e))
    assert bool((shadow[pad] == 7.0).all())
    # update AND copies from the new shadows in one launch
    for p in P:
        p.add_(0.25)
    _apply(lib, dev, swap, 1, _native.EMA_SOURCE_EMA)
    ref_apply(want, P, DECAY)
    for i, (e, w, cp, ct) in enumerate(zip(E, want, C, CT)):
        assert torch.equal(e, w), SHAPES[i]
        assert cp is None or torch.equal(cp, e.to(cp.dtype)), SHAPES[i]
        assert ct is None or torch.equal(ct, cp.t()), SHAPES[i]

    # -- dgs_adamw_ema_step: the same tensors as an AdamW table, a twin stepped by dgs_adamw_step ------------------------------
    m = torch.zeros(total, device=dev)
    v = torch.zeros(total, device=dev)
    G = [torch.zeros_like(p) for p in P]
    P2, m2, v2 = [p.clone() for p in P], m.clone(), v.clone()
    C2, CT2 = [None if c is None else torch.zeros_like(c) for c in C], [None if c is None else torch.zeros_like(c) for c in CT]

    def adamw_table(Ps, ms, vs, Cs, CTs):
        entries = []
        for (r, c, kind, tr), off, p, gr, cp, ct in zip(SHAPES, offs, Ps, G, Cs, CTs):
            t = _native.DgsAdamWTensor()
            t.p, t.g, t.m, t.v = p.data_ptr(), gr.data_ptr(), ms.data_ptr() + 4 * off, vs.data_ptr() + 4 * off
            t.rows, t.cols = r, c
            if cp is not None:
                t.copy, t.copy_kind = cp.data_ptr(), _native.OPTIM_COPY_BF16 if kind == torch.bfloat16 else _native.OPTIM_COPY_F32
            if ct is not None:
                t.copy_t = ct.data_ptr()
            entries.append(t)
        host = (_native.DgsAdamWTensor * len(entries))(*entries)
        n_tiles = lib.dgs_adamw_plan(host, len(entries))
        assert n_tiles > 0
        return _device_table(host, dev), len(entries), n_tiles

    tab, twin = adamw_table(P, m, v, C, CT), adamw_table(P2, m2, v2, C2, CT2)
    sumsq = torch.zeros(1, device=dev)
    for step in range(1, 4):
        for gr in G:
            gr.copy_(torch.randn(gr.shape, generator=g))
        sumsq.copy_(sum(gr.double().pow(2).sum() for gr in G).float().reshape(1))
        args = []
        for t in (tab, twin):
            a = _native.DgsAdamWArgs()
            a.tensors, a.n_tensors, a.n_tiles = t[0].data_ptr(), t[1], t[2]
            a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = 3e-2, 0.9, 0.99, 1e-8, 0.05
            a.bias_correction1, a.bias_correction2_sqrt = 1.0 - 0.9 ** step, (1.0 - 0.99 ** step) ** 0.5
            a.grad_sumsq, a.max_grad_norm = sumsq.data_ptr(), 0.5
            args.append(a)
        f = _native.DgsEmaFusedArgs()
        f.ema_base, f.m_base, f.one_minus_decay = shadow.data_ptr(), m.data_ptr(), 1.0 - DECAY
        assert lib.dgs_adamw_ema_step(ctypes.byref(args[0]), ctypes.byref(f), _stream(dev)) == 0
        assert lib.dgs_adamw_step(ctypes.byref(args[1]), _stream(dev)) == 0
        ref_apply(want, P, DECAY)                                      # on the kernel's own NEW p
        for i, (e, w, p, q) in enumerate(zip(E, want, P, P2)):
            assert torch.equal(e, w), (step, SHAPES[i])
            assert torch.equal(p, q), (step, SHAPES[i])                 # the EMA does not move the update
        assert torch.equal(m, m2) and torch.equal(v, v2)
        for cp, cq in zip(C + CT, C2 + CT2):
            assert cp is None or torch.equal(cp, cq)
        assert bool((shadow[pad] == 7.0).all())
    # a non-finite norm: nothing is touched, the shadows included
    keep = shadow.clone()
    sumsq.fill_(float("inf"))
    assert lib.dgs_adamw_ema_step(ctypes.byref(args[0]), ctypes.byref(f), _stream(dev)) == 0
    assert torch.equal(shadow, keep) and all(torch.equal(p, q) for p, q in zip(P, P2)) and torch.equal(m, m2)
    # null / invalid arguments
    assert lib.dgs_ema_apply(None, None) != 0
    assert lib.dgs_adamw_ema_step(None, None, None) != 0
    assert lib.dgs_adamw_ema_step(ctypes.byref(args[0]), None, _stream(dev)) != 0
    assert lib.dgs_adamw_ema_step(None, ctypes.byref(f), _stream(dev)) != 0
    bad = _native.DgsEmaArgs()
    bad.tensors, bad.n_tensors, bad.n_tiles = upd[0].data_ptr(), upd[1], upd[2]
    assert lib.dgs_ema_apply(ctypes.byref(bad), _stream(dev)) != 0      # neither an update nor copies
    if gpu:
        torch.cuda.synchronize()


def test_table_level_on_the_emulator():
    _table_level(False)


@pytest.mark.gpu
def test_table_level_on_gpu():
    _table_level(True)


def test_ema_plan_rejects_bad_tables():
    from emu_util import emu_lib
    lib = emu_lib()
    x = torch.zeros(64 * 96)
    e = _native.DgsEmaTensor()
    e.p = e.ema = x.data_ptr()
    e.rows, e.cols = 64, 96
    one = lambda: lib.dgs_ema_plan((_native.DgsEmaTensor * 1)(e), 1)
    e.copy_t = x.data_ptr()                              # a transposed copy needs both sides to be multiples of 64
    assert one() < 0
    e.copy_t = None
    assert one() == 2                                    # flat: ceil(6144 / 4096) tiles
    assert x.data_ptr() % 16 == 0
    for field in ("p", "ema"):                           # a view at an odd element offset: no 16-byte alignment for the float4 accesses
        setattr(e, field, x.data_ptr() + 4)
        assert one() < 0, field
        setattr(e, field, None)
        assert one() < 0, field
        setattr(e, field, x.data_ptr())
    e.copy, e.copy_kind = x.data_ptr() + 4, _native.OPTIM_COPY_BF16              # bf16 copy: 8-byte stores
    assert one() < 0
    e.copy = x.data_ptr() + 8
    assert one() == 2
    e.copy_kind = _native.OPTIM_COPY_F32                                           # fp32 copy: 16-byte stores
    assert one() < 0
    e.copy, e.copy_kind = None, _native.OPTIM_COPY_BF16                            # a kind without a destination
    assert one() < 0
    assert lib.dgs_ema_plan(None, 1) < 0 and lib.dgs_ema_plan((_native.DgsEmaTensor * 1)(e), 0) < 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. fused step
# ---------------------------------------------------------------------------------------------------------------------------------
def _fused_step(gpu):
    dev, lib, cfg = _where(gpu)
    a, b = _model(dev, lib, cfg), _model(dev, lib, cfg)
    ema = EMA(a, decay=0.9)
    assert ema.decay == 0.9 and ema.apply_ema_every_n_steps == 1 and ema.start_step == 0
    opts = [FusedAdamW(m, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05) for m in (a, b)]
    opts[0].attach_ema(ema)
    want = [v.detach().clone() for v in b.state_dict().values()]
    assert list(ema.shadow_state_dict()) == list(b.state_dict())
    clipped = []
    for step in range(4):
        sums = [_set_grads(m, torch.Generator().manual_seed(10 + step), 0.1 + step, dev) for m in (a, b)]
        clipped.append(float(sums[0].sqrt()) > 0.5)
        for opt, s in zip(opts, sums):
            opt.step(grad_sumsq=s, max_grad_norm=0.5)
        ref_apply(want, list(b.state_dict().values()), 0.9)
        for (k, e), w in zip(ema.shadow_state_dict().items(), want):
            assert torch.equal(e, w), (step, k)
    assert any(clipped)
    # EMA on / off does not move training: parameters, both moments, every engine copy
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    assert torch.equal(opts[0].exp_avg, opts[1].exp_avg) and torch.equal(opts[0].exp_avg_sq, opts[1].exp_avg_sq)
    da, db = a.engine().weight_destinations(), b.engine().weight_destinations()
    for n in da:
        for x, y in zip(da[n], db[n]):
            assert (x is None and y is None) or torch.equal(x, y), n
    _copies_follow(a, dict(a.named_parameters()))
    assert ema.cur_step == 4 and opts[0].step_count == 4
    assert not torch.equal(ema.shadow("transformer.0.attn.qkv.weight"), a.transformer[0].attn.qkv.weight.detach())


def test_fused_step_keeps_the_shadows_and_does_not_move_training_on_the_emulator():
    _fused_step(False)


@pytest.mark.gpu
def test_fused_step_keeps_the_shadows_and_does_not_move_training_on_gpu():
    _fused_step(True)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. schedule
# ---------------------------------------------------------------------------------------------------------------------------------
def _schedule(gpu):
    dev, lib, cfg = _where(gpu)
    m = _model(dev, lib, cfg)
    ema = EMA(m, decay=0.9, apply_ema_every_n_steps=2, start_step=3)
    opt = FusedAdamW(m, lr=3e-3, betas=(0.9, 0.99), weight_decay=0.05)
    opt.attach_ema(ema)
    want = [v.detach().clone() for v in m.state_dict().values()]
    cur, changed = None, []

    def finite_step(seed):
        nonlocal cur
        s = _set_grads(m, torch.Generator().manual_seed(seed), 1.0, dev)
        before = ema.flat.clone()
        opt.step(grad_sumsq=s, max_grad_norm=0.5)
        step = opt.step_count
        if step != cur and step >= 3 and step % 2 == 0:                   # the reference's predicate, utils/ema.py:103-104
            cur = step
            ref_apply(want, list(m.state_dict().values()), 0.9)
        changed.append(not torch.equal(before, ema.flat))
        for (k, e), w in zip(ema.shadow_state_dict().items(), want):
            assert torch.equal(e, w), (step, k)

    for i in range(5):
        finite_step(20 + i)
    assert changed == [False, False, False, True, False] and opt.step_count == 5
    # the sixth update would be selected: a NaN and an inf norm in its place change nothing and do not advance the schedule
    state = ([p.detach().clone() for p in m.parameters()], opt.exp_avg.clone(), opt.exp_avg_sq.clone(), ema.flat.clone(),
             {n: tuple(None if c is None else c.clone() for c in pair) for n, pair in m.engine().weight_destinations().items()})
    for bad in (float("nan"), float("inf")):
        for p in m.parameters():
            p.grad.fill_(float("nan"))
        opt.step(grad_sumsq=torch.tensor([bad], device=dev), max_grad_norm=0.5)
        assert all(torch.equal(p.detach(), q) for p, q in zip(m.parameters(), state[0]))
        assert torch.equal(opt.exp_avg, state[1]) and torch.equal(opt.exp_avg_sq, state[2]) and torch.equal(ema.flat, state[3])
        for n, pair in m.engine().weight_destinations().items():
            for now, was in zip(pair, state[4][n]):
                assert (now is None and was is None) or torch.equal(now, was), n
    finite_step(30)
    assert opt.step_count == 6 and opt.skipped_steps == 2 and ema.cur_step == 6 and changed[-1]


def test_schedule_and_skipped_steps_on_the_emulator():
    _schedule(False)


@pytest.mark.gpu
def test_schedule_and_skipped_steps_on_gpu():
    _schedule(True)


def test_a_parameter_without_a_gradient_is_averaged_like_the_reference_does():
    """It is absent from the AdamW table, so the launch does not see it: the same call updates its shadow with the torch expression
    (and leaves it alone, like everything else, when the gradient norm is not finite)."""
    dev, lib, cfg = _where(False)
    m = _model(dev, lib, cfg)
    ema = EMA(m, decay=0.9)
    opt = FusedAdamW(m, lr=3e-3)
    opt.attach_ema(ema)
    want = [v.detach().clone() for v in m.state_dict().values()]
    name = "image_token_decoder.linear.weight"
    for step in range(3):
        s = _set_grads(m, torch.Generator().manual_seed(40 + step), 1.0, dev)
        if step >= 1:
            dict(m.named_parameters())[name].grad = None
        opt.step(grad_sumsq=s, max_grad_norm=0.5)
        ref_apply(want, list(m.state_dict().values()), 0.9)
        for (k, e), w in zip(ema.shadow_state_dict().items(), want):
            assert torch.equal(e, w), (step, k)
    assert name not in opt._table_names and not torch.equal(ema.shadow(name), dict(m.named_parameters())[name].detach())
    keep = ema.flat.clone()
    opt.step(grad_sumsq=torch.tensor([float("nan")]), max_grad_norm=0.5)
    assert torch.equal(ema.flat, keep) and opt.step_count == 3
    # an EMA of another model is refused, not silently misapplied
    other = dn.DGSDenoiser(dict(cfg, num_layers=1), device=dev, lib=lib)
    with pytest.raises(ValueError):
        opt.attach_ema(EMA(other))
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            EMA(m, decay=bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. standalone path
# ---------------------------------------------------------------------------------------------------------------------------------
def _standalone(gpu):
    dev, lib, cfg = _where(gpu)
    m = _model(dev, lib, cfg)
    ema = EMA(m, decay=0.9)
    opt = torch.optim.AdamW(m.parameters(), lr=3e-3, betas=(0.9, 0.99), weight_decay=0.05)
    want = [v.detach().clone() for v in m.state_dict().values()]
    for step in range(3):
        _set_grads(m, torch.Generator().manual_seed(50 + step), 1.0, dev)
        opt.step()
        before = [p.detach().clone() for p in m.parameters()]
        assert ema.update(m) is True
        ref_apply(want, list(m.state_dict().values()), 0.9)
        for (k, e), w in zip(ema.shadow_state_dict().items(), want):
            assert torch.equal(e, w), (step, k)
        assert all(torch.equal(p.detach(), q) for p, q in zip(m.parameters(), before))
    assert ema.cur_step == ema.step == 3
    assert ema.update(m, step=3) is False                       # the same step again: the reference's `step != cur_step`


def test_standalone_update_after_a_torch_optimizer_on_the_emulator():
    _standalone(False)


@pytest.mark.gpu
def test_standalone_update_after_a_torch_optimizer_on_gpu():
    _standalone(True)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. swap
# ---------------------------------------------------------------------------------------------------------------------------------
def _swap(gpu):
    from dgs_amd import synth
    dev, lib, cfg = _where(gpu)
    m = _model(dev, lib, cfg)
    ema = EMA(m, decay=0.9)
    opt = FusedAdamW(m, lr=3e-2)
    opt.attach_ema(ema)
    for step in range(2):
        opt.step(grad_sumsq=_set_grads(m, torch.Generator().manual_seed(60 + step), 1.0, dev), max_grad_norm=0.5)
    batch, t = synth.make_batch(1, 64, V=4, device=dev, seed=5, with_t=True)
    run = lambda mod: mod.image_to_gaussians(batch["image"], batch["ray_o"], batch["ray_d"], t)[0]
    keys = ("xyz", "features", "scaling", "rotation", "opacity")
    with torch.no_grad():
        raw_out = run(m)
        twin = dn.DGSDenoiser(cfg, device=dev, lib=lib).to(dev)
        twin.load_state_dict(ema.shadow_state_dict())
        want = run(twin)
    raw = {k: v.detach().clone() for k, v in m.state_dict().items()}
    versions = [p._version for p in m.parameters()]
    eng = m.engine()
    moments = (opt.exp_avg.clone(), opt.exp_avg_sq.clone())
    with ema.swapped(m):
        _copies_follow(m, ema.shadow_state_dict(), "swapped")
        assert all(torch.equal(v, raw[k]) for k, v in m.state_dict().items())
        assert [p._version for p in m.parameters()] == versions and m.engine() is eng
        with torch.no_grad():
            got = run(m)
        assert all(torch.equal(got[k], want[k]) for k in keys)
        assert not all(torch.equal(got[k], raw_out[k]) for k in keys)
        with pytest.raises(RuntimeError):
            opt.step(grad_sumsq=torch.ones(1, device=dev), max_grad_norm=0.5)
        with pytest.raises(RuntimeError):
            ema.update(m)
        with pytest.raises(RuntimeError):
            with ema.swapped(m):
                pass
        _copies_follow(m, ema.shadow_state_dict(), "still swapped")       # the refused calls changed nothing
    _copies_follow(m, raw, "swapped out")
    assert all(torch.equal(v, raw[k]) for k, v in m.state_dict().items())
    assert [p._version for p in m.parameters()] == versions and m.engine() is eng
    assert torch.equal(opt.exp_avg, moments[0]) and torch.equal(opt.exp_avg_sq, moments[1]) and opt.step_count == 2
    with torch.no_grad():
        again = run(m)
    assert all(torch.equal(again[k], raw_out[k]) for k in keys)
    opt.step(grad_sumsq=_set_grads(m, torch.Generator().manual_seed(63), 1.0, dev), max_grad_norm=0.5)      # training goes on
    assert opt.step_count == 3 and ema.cur_step == 3


def test_swapped_evaluates_on_the_shadows_and_restores_on_the_emulator():
    _swap(False)


@pytest.mark.gpu
def test_swapped_evaluates_on_the_shadows_and_restores_on_gpu():
    _swap(True)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. checkpoints
# ---------------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_pair_and_resume(tmp_path):
    dev, lib, cfg = _where(False)
    m = _model(dev, lib, cfg)
    ema = EMA(m, decay=0.9, apply_ema_every_n_steps=1, start_step=1)
    opt = FusedAdamW(m, lr=3e-2)
    opt.attach_ema(ema)
    for step in range(2):
        opt.step(grad_sumsq=_set_grads(m, torch.Generator().manual_seed(70 + step), 1.0, dev), max_grad_norm=0.5)
    path = str(tmp_path / "step2.ckpt")
    first, second = ema.save_checkpoint(path, m, optimizer=opt)
    assert first == path and second == str(tmp_path / "step2-EMA.ckpt") and os.path.exists(first) and os.path.exists(second)
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == {"state_dict", "optimizer_states", "ema"} and all(k.startswith("shape_model.") for k in ck["state_dict"])
    assert ck["ema"]["cur_step"] == 2 and "shadows" not in ck["ema"]
    # the Lightning layout DGSDenoiser already reads: the -EMA file gives the averaged weights, the plain one the raw ones
    averaged = dn.DGSDenoiser(dict(cfg, pretrained_model_name_or_path=second), device=dev, lib=lib)
    plain = dn.DGSDenoiser(dict(cfg, pretrained_model_name_or_path=first), device=dev, lib=lib)
    shadows = ema.shadow_state_dict()
    for (k, v), (_, w) in zip(averaged.state_dict().items(), plain.state_dict().items()):
        assert torch.equal(v, shadows[k]), k
        assert torch.equal(w, m.state_dict()[k]), k
    assert not torch.equal(averaged.transformer[0].attn.qkv.weight, plain.transformer[0].attn.qkv.weight)

    def fresh():
        mm = _model(dev, lib, cfg, seed=9)
        return mm, EMA(mm), FusedAdamW(mm, lr=1.0)

    # resume from the plain path, sibling present: weights, optimizer state, shadows and the schedule's state
    m2, e2, o2 = fresh()
    e2.load_checkpoint(path, optimizer=o2)
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in m2.state_dict().items())
    assert all(torch.equal(v, shadows[k]) for k, v in e2.shadow_state_dict().items())
    assert e2.cur_step == 2 and e2.decay == 0.9 and e2.start_step == 1 and o2.step_count == 2 and torch.equal(o2.exp_avg, opt.exp_avg)
    assert o2.param_groups[0]["lr"] == 3e-2
    # resume from the -EMA path: the averaged weights ARE the main weights, the shadows restart from them
    m3, e3, _ = fresh()
    e3.load_checkpoint(second)
    assert all(torch.equal(v, shadows[k]) for k, v in m3.state_dict().items())
    assert all(torch.equal(v, m3.state_dict()[k]) for k, v in e3.shadow_state_dict().items())
    # no sibling: a warning, and restarted shadows
    os.remove(second)
    m4, e4, _ = fresh()
    with pytest.warns(UserWarning, match="unable to find the associated EMA weights"):
        e4.load_checkpoint(path)
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in m4.state_dict().items())
    assert all(torch.equal(v, m4.state_dict()[k]) for k, v in e4.shadow_state_dict().items())
    with pytest.raises(ValueError):
        ema.save_checkpoint(str(tmp_path / "weights.pt"), m)
    # state_dict / load_state_dict round trip
    sd = ema.state_dict()
    assert set(sd) == {"cur_step", "step", "decay", "apply_ema_every_n_steps", "start_step", "shadows"}
    m5, e5, _ = fresh()
    e5.load_state_dict(sd)
    assert e5.cur_step == 2 and e5.decay == 0.9 and e5.start_step == 1 and torch.equal(e5.flat, ema.flat)
    sd["shadows"].pop("gaussians_pos_embedding")
    with pytest.raises(ValueError):
        e5.load_state_dict(sd)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. trainer
# ---------------------------------------------------------------------------------------------------------------------------------
def _trainer_inputs(dev):
    import numpy as np
    from dgs_amd import cameras, synth
    batch, t = synth.make_batch(1, 64, V=4, device=dev, seed=5, with_t=True)
    rc2w = torch.tensor(np.stack([cameras.ring_cameras(2, phase_deg=5.0)])).to(dev)
    rk = torch.tensor(cameras.default_fxfycxcy(64)).expand(1, 2, 4).contiguous().to(dev)
    target = torch.rand(1, 2, 3, 64, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    return batch, t, target, rc2w, rk


def _trainer_run(kind, dev, inputs, steps=2):
    from dgs_amd.train import DataParallelTrainer
    batch, t, target, rc2w, rk = inputs
    m = dn.DGSDenoiser(GPU_CFG, device=dev)
    m.reset_parameters(seed=2)
    m = m.to(dev)
    m.train()
    if kind == "dgs_fused":
        opt, clip = FusedAdamW(m, lr=1e-3), 0.5
    else:
        opt, clip = torch.optim.AdamW(m.parameters(), lr=1e-3, foreach=True), None
    ema = EMA(m, decay=0.9)
    want = [v.detach().clone() for v in m.state_dict().values()]
    snaps = []
    with DataParallelTrainer(m, opt, max_grad_norm=clip, ema=ema) as tr:
        assert tr.ema is ema and (opt._ema is ema if kind == "dgs_fused" else True)
        for _ in range(steps):
            tr.step(batch, t, target, rc2w, rk)
            snaps.append([v.detach().clone() for v in m.state_dict().values()])
        for snap in snaps:                                            # the reference loop replayed from the parameter snapshots
            ref_apply(want, snap, 0.9)
        for (k, e), w in zip(ema.shadow_state_dict().items(), want):
            assert torch.equal(e, w), (kind, k)
        assert sum(not torch.equal(x, y) for x, y in zip(snaps[0], snaps[1])) > 0.9 * len(want), kind
        _copies_follow(m, dict(m.named_parameters()), kind)
        render = lambda: m.render_gaussians(m.image_to_gaussians(batch["image"], batch["ray_o"], batch["ray_d"], t)[0], rc2w, rk, 64, 64)
        with torch.no_grad():
            outside = render().clone()
            with tr.evaluate():
                inside = render().clone()
                with pytest.raises(RuntimeError):
                    tr.step(batch, t, target, rc2w, rk)
            after = render().clone()
        assert not torch.equal(inside, outside) and torch.equal(after, outside), kind
        _copies_follow(m, dict(m.named_parameters()), kind + " after evaluate")
        tr.step(batch, t, target, rc2w, rk)                           # training goes on after an evaluation
    return ema.flat.clone()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["dgs_fused", "torch_foreach"])
def test_trainer_keeps_the_shadows_and_evaluates_on_them(kind):
    dev = torch.device("cuda:0")
    _trainer_run(kind, dev, _trainer_inputs(dev))


@pytest.mark.gpu
def test_two_trainer_runs_with_an_ema_end_with_bit_identical_shadows():
    dev = torch.device("cuda:0")
    inputs = _trainer_inputs(dev)
    a, b = _trainer_run("dgs_fused", dev, inputs), _trainer_run("dgs_fused", dev, inputs)
    assert torch.equal(a, b)


@pytest.mark.gpu
def test_evaluate_without_an_ema_is_a_no_op():
    from dgs_amd.train import DataParallelTrainer
    dev = torch.device("cuda:0")
    m = dn.DGSDenoiser(GPU_CFG, device=dev).to(dev)
    with DataParallelTrainer(m, FusedAdamW(m, lr=1e-3)) as tr:
        before = {n: (c.clone(), None if ct is None else ct.clone()) for n, (c, ct) in m.engine().weight_destinations().items()}
        with tr.evaluate():
            pass
        for n, (c, ct) in m.engine().weight_destinations().items():
            assert torch.equal(c, before[n][0]) and (ct is None or torch.equal(ct, before[n][1]))


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_symbol_of_dgs_ema_h_is_exported_and_the_structs_match():
    from dgs_amd import build as build_mod
    build_mod.build_hip()
    lib = _native.lib()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "dgs_ema.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(dgs_[a-z0-9_]+)\s*\(", txt)))
    assert names and sorted(_native.EMA_SYMBOLS) == names, sorted(set(names) ^ set(_native.EMA_SYMBOLS))
    for n in names:
        assert hasattr(lib, n), f"{n} declared in dgs_ema.h but not exported"
    # dgs_optim.h did not grow: the fused entry is declared in the new header
    assert "dgs_adamw_ema_step" not in open(os.path.join(INC, "dgs_optim.h")).read()
    structs = ["DgsEmaFusedArgs", "DgsEmaTensor", "DgsEmaArgs", "DgsAdamWTensor", "DgsAdamWArgs"]
    src = '#include <stdio.h>\n#include "dgs_ema.h"\nint main(){' + "".join(f'printf("%zu\\n", sizeof({s}));' for s in structs) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I" + INC, c, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    for s, n in zip(structs, sizes):
        assert ctypes.sizeof(getattr(_native, s)) == n, (s, ctypes.sizeof(getattr(_native, s)), n)
    assert (_native.EMA_SOURCE_NONE, _native.EMA_SOURCE_P, _native.EMA_SOURCE_EMA) == tuple(
        int(re.search(rf"#define DGS_EMA_SOURCE_{k} (\d)", txt).group(1)) for k in ("NONE", "P", "EMA"))


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. what the swap and the binding to one model refuse
# ---------------------------------------------------------------------------------------------------------------------------------
def test_swapped_refuses_what_would_silently_end_it_and_the_ema_is_bound_to_its_model(tmp_path):
    dev, lib, cfg = _where(False)
    m = _model(dev, lib, cfg)
    ema = EMA(m, decay=0.9)
    ema.flat.mul_(0.5)                                               # shadows that differ from the weights
    sd = ema.state_dict()
    with ema.swapped(m):
        with pytest.raises(RuntimeError):
            m.refresh_engine_weights()
        m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})      # moves the version counters
        with pytest.raises(RuntimeError):
            m.engine()                                               # would refresh the copies from the raw weights
        for call in (ema.restart_from, lambda: ema.load_state_dict(sd)):
            with pytest.raises(RuntimeError):
                call()
        dst = m._engine.weight_destinations()
        for n, (copy, _) in dst.items():                             # still the averaged weights
            assert torch.equal(copy.reshape(ema.shadow(n).shape), ema.shadow(n).to(copy.dtype)), n
    _copies_follow(m, dict(m.named_parameters()), "after the block")  # engine() works again and follows the parameters
    other = _model(dev, lib, cfg, seed=3)
    for call in (lambda: ema.update(other), lambda: ema.restart_from(other), lambda: ema.save_checkpoint(str(tmp_path / "a.ckpt"), other),
                 lambda: ema.swapped(other).__enter__()):
        with pytest.raises(ValueError):
            call()
    assert ema.update(m) is True and ema.update() is True            # the model it was built for, named or not
    # the sibling's name: the file's own extension only; an -EMA path has no sibling
    assert EMA.ema_path("/runs/x.ckpt/last.ckpt") == "/runs/x.ckpt/last-EMA.ckpt"
    for bad in ("/runs/last-EMA.ckpt", "/runs/last.pt"):
        with pytest.raises(ValueError):
            EMA.ema_path(bad)
    with pytest.raises(ValueError):
        ema.save_checkpoint(str(tmp_path / "b-EMA.ckpt"), m)


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. data parallel: the shadows follow the init-time broadcast of the parameters
# ---------------------------------------------------------------------------------------------------------------------------------
def _broadcast_worker(rank, world, port, out):
    import sys
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.join(here, "..", "open-diffusiongs_amd"), os.path.join(here, "..")):
        sys.path.insert(0, os.path.abspath(p))
    import torch.distributed as dist
    from dgs_amd.parallel import init_distributed
    from dgs_amd.train import DataParallelTrainer
    from emu_util import emu_lib
    init_distributed(backend="gloo")
    cfg = dict(width=256, in_channels=9, patch_size=8, num_layers=1)
    results = {}
    for case in ("fresh", "resumed"):
        m = dn.DGSDenoiser(cfg, device="cpu", lib=emu_lib())
        m.reset_parameters(seed=1 + rank)                            # every rank constructed with weights of its own
        ema = EMA(m, decay=0.9)                                      # ... and cloned THOSE
        mine = {k: v.detach().clone() for k, v in m.state_dict().items()}
        if case == "resumed":                                        # shadows that are not the weights (a loaded -EMA sibling), a schedule state
            ema.flat.add_(1.0 + rank)
            ema.cur_step, ema.step = 5 + rank, 5 + rank
        with DataParallelTrainer(m, torch.optim.SGD(m.parameters(), lr=0.0), bucket_bytes=1 << 20, ema=ema) as tr:
            assert tr.broadcast_bytes > 4 * sum(p.numel() for p in m.parameters())       # parameters and shadows
        sd = m.state_dict()
        moved = any(not torch.equal(sd[k], mine[k]) for k in sd)     # rank 0 keeps its weights, the others got rank 0's
        add = 1.0 if case == "resumed" else 0.0                      # rank 0's shadows: its weights (+ 1.0)
        ok = all(torch.equal(ema.shadow(k), sd[k] + add) for k in sd)
        results[case] = (moved, ok, ema.cur_step, ema.step, float(ema.flat.double().sum()))
    out.put((rank, results))
    dist.barrier()
    dist.destroy_process_group()


def test_shadows_follow_the_init_time_broadcast_on_two_ranks():
    """The EMA exists before the trainer, so before rank `broadcast_from`'s parameters replace every other rank's: without a broadcast
    of the shadows a rank would average from its discarded initial weights (37 % of the shadow after 10,000 steps at decay 0.9999)."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_broadcast_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=170) for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for case in ("fresh", "resumed"):
        (moved0, ok0, cur0, step0, sum0), (moved1, ok1, cur1, step1, sum1) = got[0][case], got[1][case]
        assert not moved0 and moved1, case
        assert ok0 and ok1 and sum0 == sum1, (case, sum0, sum1)
        assert (cur0, step0) == (cur1, step1) == ((5, 5) if case == "resumed" else (None, 0)), case
