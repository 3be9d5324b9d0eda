"""The DiT row kernels (csrc/dit_elementwise.hip, csrc/dit_backward_elementwise.hip) one by one against fp64: LayerNorm + modulate, the
<= 16-row Linear, their backward kernels, the gate multiply with its column sums, the token scatter / gather.  Cases, seeded inputs,
fp64 references with their derived error bars, guarded launches and one check_* function per kernel taking (lib, device, ...).
Shared by test_dit_rowkernels_emu.py (CPU emulator build), test_dit_rowkernels_gpu.py (MI355X) and tools/dit_rowkernel_error.py.

Harness (every case): inputs are seeded on the CPU and rounded to their storage type before the reference sees them; the reference is
the operation's plain expression in fp64 torch; every output and scratch buffer is a view into a larger allocation with 16 KiB of 0xA5
bytes in front and behind (checked bit for bit after the call; the widest row here is 8 KiB); scratch slabs start as NaN, written
outputs as 7.0 (the sums are written, not accumulated); `before` (the GPU tests: poison_lds) runs in front of every launch; every call
runs twice and the second result must equal the first bit for bit.

Bars (none comes from the code under test).  u = 2^-24, ulp = 2^-23.
  fp32 sums    |got - ref64| <= depth u sum|terms| per element, depth = the longest chain of additions (and the term's own roundings) a
               term passes through in the kernel's stated order; sum|terms| in fp64.  The depth formulas stand next to each reference.
               A SiLU in front of or behind the sum adds 4 ulp per activated term (__expf).
  LayerNorm    the same bound carried through mean, variance and rstd PER ROW (ln_stats): a row with mean 1000 and spread 3 has an
               inherent fp32 error ~40 x that of its neighbours, a tensor-wide bar would be too loose or too tight.
  bf16 outputs each element equals the round-to-nearest-even bf16 of the fp64 reference, except where the reference lies within the fp32
               bound of a rounding midpoint: there either neighbour passes; at most 0.5 % of a tensor may take that exception.
  copies       bit-equal (dyT against dy, in-place against out-of-place).
Every check appends (kernel, case, output, error, bar, error / bar, exception share) to RECORDS; tools/dit_rowkernel_error.py writes
them to profiles/dit_rowkernels_parity.txt.

Out of scope -- no C entry point reaches them alone, they stay covered through the whole-model tests only: the single-workgroup `+=`
path of layernorm_backward_kernel, ROWLINEAR_DW_ROWS launches, embed_patchify_kernel, gaussians_kernel and gaussians_backward_kernel,
timestep_freq_kernel, transpose_kernel, the two colsum kernels.  (No test-only exports are added to the ABI for them.)"""
import ctypes
import math
import os

import torch

from dgs_amd import _native

U, ULP = 2.0 ** -24, 2.0 ** -23
INVALID = -1                               # DGS_ERR_INVALID_ARGUMENT (include/dgs_raster.h)
GUARD_BYTE, GUARD_BYTES = 0xA5, 1 << 14    # the pattern of dit_util.guard_arena
EXCEPTION_CAP = 0.005
RECORDS = []
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def ceil_div(a, b):
    return (a + b - 1) // b


# ---- guarded launches ---------------------------------------------------------------------------------------------------------------
class Arena:
    """Output and scratch buffers of one call, each carved out of a larger allocation between two bands of 0xA5 bytes."""

    def __init__(self, device):
        self.device, self.bufs = torch.device(device), []

    def take(self, shape, dtype, fill):
        shape = tuple(int(s) for s in shape)
        n = math.prod(shape) * torch.empty(0, dtype=dtype).element_size()
        big = torch.full((GUARD_BYTES + (n + 15) // 16 * 16 + GUARD_BYTES,), GUARD_BYTE, dtype=torch.uint8, device=self.device)
        inner = big[GUARD_BYTES:GUARD_BYTES + n].view(dtype).view(shape)
        assert inner.data_ptr() % 16 == 0
        inner.fill_(fill)
        self.bufs.append((big, n))
        return inner

    def check(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        dirty = sum(int((b[:GUARD_BYTES] != GUARD_BYTE).sum()) + int((b[GUARD_BYTES + n:] != GUARD_BYTE).sum()) for b, n in self.bufs)
        assert dirty == 0, f"{dirty} guard bytes overwritten"


def call(lib, fn, struct, device, before=None, expect=0, **kw):
    """The C entry point `fn` with `struct` filled from kw (tensors as pointers), on the device's current stream."""
    a = struct()
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            setattr(a, k, v.data_ptr())
        elif v is not None:
            setattr(a, k, v)
    dev = torch.device(device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
    if before:
        before()
    rc = getattr(lib, fn)(ctypes.byref(a), stream)
    assert rc == expect, (fn, rc, expect)


def bits(t):
    return t.contiguous().view(_INT[t.element_size()])


def bit_equal(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def twice(run):
    first, second = run(), run()
    for k in first:
        assert bit_equal(first[k], second[k]), f"{k}: two identical launches differ"
    return first


def all_equal(t, value):
    return bool((t == value).all())


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def _record(kernel, case, name, err, bar, ratio, share):
    RECORDS.append((kernel, case, name, err, bar, ratio, share))


def f32_ratio(got, ref, bar):
    err = (got.double() - ref).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / bar.expand_as(err).clamp_min(1e-300)), err


def check_f32(kernel, case, name, got, ref, bar):
    assert bool(torch.isfinite(got).all()), (kernel, case, name, "not finite")
    ratio, err = f32_ratio(got, ref, bar)
    i = int(ratio.argmax())
    r = float(ratio.flatten()[i])
    _record(kernel, case, name, float(err.flatten()[i]), float(bar.expand_as(err).flatten()[i]), r, None)
    assert r <= 1.0, (kernel, case, name, "error / bar", r, "at", i)
    return r


def bf16_neighbours(ref):
    """The two bf16 values around an fp64 value: towards zero and away from it."""
    b = ref.float().view(torch.int32) & -65536
    return b.view(torch.float32).double(), (b + 65536).view(torch.float32).double()


def bf16_cell(got):
    """[lo, hi] of the values that round to the bf16 `got`: from the midpoint towards its lower neighbour to the one towards its upper."""
    b = got.contiguous().view(torch.int16).to(torch.int32)
    mag, neg = b & 0x7FFF, (b & 0x8000) != 0
    val = lambda m: (m << 16).view(torch.float32).double()
    away = (val(mag) + val(mag + 1)) / 2
    toward = torch.where(mag > 0, (val(mag) + val((mag - 1).clamp_min(0))) / 2, -val(torch.ones_like(mag)) / 2)
    return torch.where(neg, -away, toward), torch.where(neg, -toward, away)


def bf16_verdict(got, ref, bar):
    """(bad, took, ratio).  An element passes when it is the round-to-nearest-even bf16 of ref, or when a rounding midpoint next to it
    lies within `bar` of ref (either neighbour of such a midpoint passes: the values within the fp32 bound of ref do not all round to
    the same bf16).  Where the bound exceeds a bf16 step -- elements near zero of a row with a large mean -- that is more than one
    midpoint.  took: passed without being the nearest; ratio: |got - ref| / (half a bf16 step + bar)."""
    g = got.float().double()
    want = ref.float().to(torch.bfloat16).float().double()
    lo, hi = bf16_neighbours(ref)
    cell_lo, cell_hi = bf16_cell(got)
    exact = g == want
    took = ~exact & (ref + bar >= cell_lo) & (ref - bar <= cell_hi)
    return ~exact & ~took, took, (g - ref).abs() / ((hi - lo).abs() / 2 + bar)


def check_bf16(kernel, case, name, got, ref, bar):
    assert bool(torch.isfinite(got.float()).all()), (kernel, case, name, "not finite")
    bar = bar.expand_as(ref)
    bad, took, ratio = bf16_verdict(got, ref, bar)
    share = float(took.double().mean())
    i = int(ratio.argmax())
    _record(kernel, case, name, float((got.float().double() - ref).abs().flatten()[i]), float(bar.flatten()[i]), float(ratio.flatten()[i]), share)
    assert not bool(bad.any()), (kernel, case, name, int(bad.sum()), "elements are not the nearest bf16 of the reference; first", int(bad.flatten().nonzero()[0]))
    assert share <= EXCEPTION_CAP, (kernel, case, name, "share of either-neighbour exceptions", share)
    return share


# ---- LayerNorm + modulate -----------------------------------------------------------------------------------------------------------
LN_WIDTHS = (256, 512, 768, 1024, 2048)
LN_SHAPES = ((21, 7), (19, 7))             # (rows, rows_per_batch): idle waves in each sample's last workgroup; a short last sample
LN_EPS = (1e-6, 1e-5)
OUTLIER_MEAN, SPREAD = 1000.0, 3.0
# seed of a case = LN_SEED + width + rows.  What a one-pass fp32 variance loses on the mean-1000 row is a matter of rounding luck (0.5 to
# 158 bars over the draws): 1100 is the first of 100, 1100, 2100, ... at which that mutant clears 2 bars at every width, shape and eps
# (asserted by test_layernorm_bars_catch_the_mutants), so that the kernel tests run on inputs on which the bar can tell it apart.
LN_SEED = 1100


def ln_inputs(rows, width, B, seed, device, mod_cols=6):
    """x with spread 3, row rows // 2 with mean 1000; weight around 1; shift / scale as column slices of one [B, mod_cols width] tensor
    that differ by O(1) between samples."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, width, generator=g) * SPREAD + 0.5
    x[rows // 2] += OUTLIER_MEAN
    w = 1.0 + 0.2 * torch.randn(width, generator=g)
    mod = torch.randn(B, mod_cols * width, generator=g) + 1.5 * torch.arange(B, dtype=torch.float32)[:, None]
    return x.to(device), w.to(device), mod.to(device)


def ln_stats(x, eps):
    """fp64 mean / rstd / normalised row of x [rows, width], with the bound of the kernel's fp32 error on each.
    depth d = 2 ((a + b) + (c + d) of a float4) + VPL (a lane's float4s, one after the other) + 6 (wave levels) + 1 (the division).
    mean: |dm| <= d u sum|x| / W.  centred: c~ = (c - dm)(1 + e), and sum (c - dm)^2 = sum c^2 + W dm^2 because sum c = 0, so
    var~ <= (var + dm^2)(1 + (d + 4) u): the rounding of c twice, of the square, the chain.  rstd: half the relative error of var + eps,
    + 4 u (the addition of eps, rsqrtf, the division by W).  n = c~ rstd~."""
    width = x.shape[-1]
    d = 2 + width // 256 + 6 + 1
    mean = x.mean(-1, keepdim=True)
    dm = d * U * x.abs().sum(-1, keepdim=True) / width
    c = x - mean
    var = (c * c).mean(-1, keepdim=True)
    dvar = dm * dm + (d + 4) * U * (var + dm * dm)
    rstd = (var + eps).rsqrt()
    rel = 0.5 * dvar / (var + eps) + 4 * U
    n = c * rstd
    en = rstd * (dm + U * c.abs()) + n.abs() * (rel + U)
    return dict(n=n, en=en, rstd=rstd, rel=rel)


def ref_layernorm(x, weight, shift, scale, rpb, eps):
    """(y, bar) in fp64.  y = LN(x) [* weight] [* (1 + scale[b]) + shift[b]], b = row // rpb; one u per fp32 operation on the way."""
    st = ln_stats(x, eps)
    y, e = st["n"], st["en"]
    if weight is not None:
        y = y * weight
        e = e * weight.abs() + U * y.abs()
    if shift is not None:
        b = torch.arange(x.shape[0], device=x.device) // rpb
        m1 = 1.0 + scale[b]
        t = y * m1
        y = t + shift[b]
        e = e * m1.abs() + 2 * U * t.abs() + U * y.abs()
    return y, e


def check_layernorm(lib, device, widths=LN_WIDTHS, shapes=LN_SHAPES, before=None):
    A = _native.DgsDitLayerNormArgs
    for width in widths:
        for rows, rpb in shapes:
            B = ceil_div(rows, rpb)
            x, w, mod = ln_inputs(rows, width, B, LN_SEED + width + rows, device)
            shift, scale = mod[:, :width], mod[:, width:2 * width]
            x64, w64, sh64, sc64 = x.double(), w.double(), shift.double(), scale.double()
            for eps in LN_EPS:
                for form in range(8):
                    use_w, use_m, f32 = bool(form & 1), bool(form & 2), bool(form & 4)

                    def run():
                        ar = Arena(device)
                        out = ar.take((rows, width), torch.float32 if f32 else torch.bfloat16, 7.0)
                        call(lib, "dgs_dit_layernorm", A, device, before, rows=rows, width=width, x=x, weight=w if use_w else None,
                             shift=shift if use_m else None, scale=scale if use_m else None, mod_stride=6 * width, rows_per_batch=rpb,
                             eps=eps, out=out, out_f32=int(f32))
                        ar.check()
                        return {"out": out.clone()}
                    got = twice(run)["out"]
                    ref, bar = ref_layernorm(x64, w64 if use_w else None, sh64 if use_m else None, sc64 if use_m else None, rpb, eps)
                    case = f"width {width} rows {rows}/{rpb}"
                    (check_f32 if f32 else check_bf16)("layernorm", case, "out f32" if f32 else "out bf16", got, ref, bar)
        # the input LayerNorm's form: f32, weight only, out == x -- bit-equal to out of place
        rows, rpb = shapes[0]
        x, w, mod = ln_inputs(rows, width, ceil_div(rows, rpb), LN_SEED + width + rows, device)
        res = {}
        for inplace in (False, True):
            ar = Arena(device)
            out = ar.take((rows, width), torch.float32, 7.0)
            if inplace:
                out.copy_(x)
            call(lib, "dgs_dit_layernorm", A, device, before, rows=rows, width=width, x=out if inplace else x, weight=w, mod_stride=0,
                 rows_per_batch=0, eps=1e-6, out=out, out_f32=1)
            ar.check()
            res[inplace] = out.clone()
        assert bit_equal(res[True], res[False]), ("layernorm in place", width)
        # the upsampler head's form: rows = rows_per_batch = 2, x at an offset inside a larger tensor, one sample's modulation
        xs = x[5:7]
        assert xs.data_ptr() != x.data_ptr()

        def run_head():
            ar = Arena(device)
            out = ar.take((2, width), torch.float32, 7.0)
            call(lib, "dgs_dit_layernorm", A, device, before, rows=2, width=width, x=xs, weight=w, shift=mod[:1, :width],
                 scale=mod[:1, width:2 * width], mod_stride=6 * width, rows_per_batch=2, eps=1e-6, out=out, out_f32=1)
            ar.check()
            return {"out": out.clone()}
        ref, bar = ref_layernorm(xs.double(), w.double(), mod[:1, :width].double(), mod[:1, width:2 * width].double(), 2, 1e-6)
        check_f32("layernorm", f"width {width} rows 2/2 offset x", "out f32", twice(run_head)["out"], ref, bar)


# ---- row-linear ---------------------------------------------------------------------------------------------------------------------
RL_MS = (1, 2, 3, 4, 5, 8, 9, 16)
RL_NS = (14, 33, 37, 6144 + 14)
RL_KS = (256, 512, 1024, 2048)             # 2048 for M <= 8 (16 rows of 2048 floats are 128 KiB of LDS); M = 16, K = 1024 is the 64 KiB boundary


def silu64(v):
    return v * torch.sigmoid(v)


def dsilu64(v):
    s = torch.sigmoid(v)
    return s * (1.0 + v * (1.0 - s))


def rowlinear_depth(K):
    """8 per 512-wide K step of a lane (seven additions among its 8 products, one into the accumulator), 6 wave levels, the product's
    own rounding and the bias."""
    return 8 * ceil_div(K, 512) + 6 + 2


def ref_rowlinear_sum(x, W, silu_in):
    """(acc, sum|terms|) of sum_k act(x[m, k]) W[n, k] in fp64."""
    xa = silu64(x) if silu_in else x
    return xa @ W.t(), xa.abs() @ W.abs().t()


def ref_rowlinear_finish(acc, S, K, bias, silu_in, silu_out):
    d = rowlinear_depth(K)
    if bias is not None:
        acc, Sb = acc + bias, S + bias.abs()
    else:
        Sb = S
    e = d * U * Sb + (4 * ULP * S if silu_in else 0.0)
    if silu_out:
        y = silu64(acc)
        return y, dsilu64(acc).abs() * e + 0.5 * e * e + 4 * ULP * y.abs()
    return acc, e


def ref_rowlinear(x, W, bias, silu_in, silu_out):
    acc, S = ref_rowlinear_sum(x, W, silu_in)
    return ref_rowlinear_finish(acc, S, x.shape[1], bias, silu_in, silu_out)


def rowlinear_inputs(M, N, K, device):
    g = torch.Generator().manual_seed(7 * N + K)
    W = (torch.randn(N, K, generator=g) * 0.1).to(torch.bfloat16)
    bias = torch.randn(N, generator=g)
    x = torch.randn(16, K, generator=g)[:M].contiguous()
    return x.to(device), W.to(device), bias.to(device)


def check_rowlinear(lib, device, Ms=RL_MS, Ns=RL_NS, Ks=RL_KS, before=None):
    A = _native.DgsDitRowLinearArgs
    for N in Ns:
        for K in Ks:
            W64 = None
            for M in Ms:
                if K > 1024 and M > 8:
                    continue
                x, W, bias = rowlinear_inputs(M, N, K, device)
                W64 = W.double() if W64 is None else W64
                for silu_in in (0, 1):
                    acc, S = ref_rowlinear_sum(x.double(), W64, silu_in)
                    for use_b in (0, 1):
                        for silu_out in (0, 1):
                            def run():
                                ar = Arena(device)
                                out = ar.take((M, N), torch.float32, 7.0)
                                call(lib, "dgs_dit_rowlinear", A, device, before, M=M, N=N, K=K, x=x, silu_input=silu_in, W=W,
                                     bias=bias if use_b else None, silu_output=silu_out, out=out)
                                ar.check()
                                return {"out": out.clone()}
                            ref, bar = ref_rowlinear_finish(acc, S, K, bias.double() if use_b else None, silu_in, silu_out)
                            check_f32("rowlinear", f"M {M} N {N} K {K}", "out", twice(run)["out"], ref, bar)


# ---- LayerNorm backward -------------------------------------------------------------------------------------------------------------
LNB_WIDTHS = (256, 512, 1024)
LNB_BS = (1, 3)
LNB_RPBS = (5, 17, 24, 64)                 # fewer rows than waves; wave 0 gets a third row; first divisor >= 16 on 256 CUs; 4 blocks per sample
LNB_MASKS = tuple(range(8))                # bit 0: dshift, bit 1: dscale, bit 2: dweight
LNB_TRAIN = (4, 4224, 1024)                # the training partition on 256 CUs: 66 rows per block, 256 blocks, 64 slots per sample


def ln_rows_per_block(rows_per_batch, rows, ncu):
    """The rule of csrc/dit_kernels.h, restated: the smallest divisor of the sample's rows, >= 16 and >= rows / CUs, at most 8 x that;
    32 (or the whole sample) when there is none or the CU count is unknown."""
    if ncu > 0 and rows > 0:
        want = max(16, ceil_div(rows, ncu))
        for d in range(want, min(rows_per_batch, 8 * want) + 1):
            if rows_per_batch % d == 0:
                return d
    return 32 if rows_per_batch % 32 == 0 else rows_per_batch


def compute_units(device):
    dev = torch.device(device)
    if dev.type == "cuda":
        return torch.cuda.get_device_properties(dev).multi_processor_count
    return int(os.environ.get("DGS_EMU_CUS", "0"))


def ref_ln_backward(x, dh, weight, scale_rows, eps, dx_in, B, rpb, rpblk):
    """fp64 backward of h = LN(x) w (1 + scale) + shift with bars.  Column sums: a term passes through ceil(rows_per_block / 8) additions in
    its wave's registers, 8 in the workgroup's wave-order sum, ceil(slots / 4) + 2 in the slab reduce: depth = the sum of those; a term
    g n w carries the error of n (ln_stats) and its products' roundings.  dx = rstd (dn - mean(dn) - n mean(dn n)) [+ dx_in]: the two
    row means have the depth of the statistics."""
    rows, width = x.shape
    st = ln_stats(x, eps)
    n, en, rstd, rel = st["n"], st["en"], st["rstd"], st["rel"]
    w = weight if weight is not None else torch.ones(width, dtype=torch.float64, device=x.device)
    m1 = 1.0 + scale_rows if scale_rows is not None else torch.ones_like(x)
    slots = rpb // rpblk
    depth_b = ceil_div(rpblk, 8) + 8 + ceil_div(slots, 4) + 2          # per sample: dshift, dscale
    depth_w = ceil_div(rpblk, 8) + 8 + ceil_div(B * slots, 4) + 2      # over all rows: dweight
    per_b = lambda t: t.reshape(B, rpb, width).sum(1)
    out = {}
    out["dshift"] = (per_b(dh), depth_b * U * per_b(dh.abs()))
    t = dh * n * w
    out["dscale"] = (per_b(t), (depth_b + 2) * U * per_b(t.abs()) + per_b((dh * w).abs() * en))
    t = dh * m1 * n
    out["dweight"] = (t.sum(0), (depth_w + 3) * U * t.abs().sum(0) + ((dh * m1).abs() * en).sum(0))
    d = 2 + width // 256 + 6 + 1
    dn = dh * m1 * w
    e_dn = 3 * U * dn.abs()
    mean = lambda t: t.mean(-1, keepdim=True)
    m1s, p = mean(dn), dn * n
    e_m1s = d * U * mean(dn.abs()) + mean(e_dn)
    m2s = mean(p)
    e_m2s = d * U * mean(p.abs()) + mean(e_dn * n.abs() + dn.abs() * en + U * p.abs())
    inner = dn - m1s - n * m2s
    e_in = e_dn + e_m1s + en * m2s.abs() + n.abs() * e_m2s + U * (n * m2s).abs() + 2 * U * (dn.abs() + m1s.abs() + (n * m2s).abs())
    dx = rstd * inner
    e_dx = rstd * e_in + dx.abs() * (rel + U)
    if dx_in is not None:
        dx = dx + dx_in
        e_dx = e_dx + U * dx.abs()
    out["dx"] = (dx, e_dx)
    return out


def lnb_inputs(B, rpb, width, dh_f32, seed, device):
    """x as ln_inputs; dh = 0.5 + rand (same-signed terms: a dropped row of T moves a column sum by at least 1 / (3 T))."""
    rows = B * rpb
    x, w, mod = ln_inputs(rows, width, B, seed, device, mod_cols=3)
    g = torch.Generator().manual_seed(seed + 1)
    dh = 0.5 + torch.rand(rows, width, generator=g)
    dh = dh if dh_f32 else dh.to(torch.bfloat16)
    dx_in = torch.randn(rows, width, generator=g)
    return x, w, mod, dh.to(device), dx_in.to(device)


def lnb_configs(shape_idx, masks):
    """Per shape one config per column-sum subset; dh type, the four weight / scale forms and the three dx_in modes rotate so that over
    the 8 shapes of a width every (subset, dh type, weight, scale) combination and every (subset, dx_in mode) pair is met."""
    for j, mask in enumerate(masks):
        i = j + shape_idx
        yield dict(mask=mask, dh_f32=i % 2, weight=bool((i // 2) & 1), scale=bool((i // 4) & 1), dxin=("in", "none", "inplace")[(i + j) % 3])


def run_ln_backward(lib, device, before, x, dh, dh_f32, w, mod, eps, dx_in, mode, mask, B, rpb, width, ncu):
    """One guarded dgs_dit_layernorm_backward; mod [B, 3 width]: scale = its middle third; dshift / dscale go to the first two thirds of a
    [B, 3 width] output whose last third -- and every third not requested -- must stay 7.0; the scratch size is restated from the rule."""
    rows = B * rpb
    rpblk = ln_rows_per_block(rpb, rows, ncu)
    blocks = ceil_div(rows, rpblk)
    nb = int(lib.dgs_dit_layernorm_backward_scratch_bytes(rows, width, rpb))
    assert nb == blocks * 3 * width * 4, (nb, blocks, rpblk, ncu)
    ar = Arena(device)
    dx = ar.take((rows, width), torch.float32, 7.0)
    dmod = ar.take((B, 3 * width), torch.float32, 7.0)
    dw = ar.take((width,), torch.float32, 7.0)
    scratch = ar.take((blocks, 3 * width), torch.float32, float("nan"))
    if mode == "inplace":
        dx.copy_(dx_in)
    call(lib, "dgs_dit_layernorm_backward", _native.DgsDitLayerNormBackwardArgs, device, before, rows=rows, width=width, x=x, dh=dh,
         dh_f32=int(dh_f32), weight=w, scale=mod[:, width:] if mod is not None else None, mod_stride=3 * width, rows_per_batch=rpb, eps=eps,
         dx_in={"in": dx_in, "none": None, "inplace": dx}[mode], dx_out=dx, dshift=dmod if mask & 1 else None,
         dscale=dmod[:, width:] if mask & 2 else None, dweight=dw if mask & 4 else None, scratch=scratch, scratch_bytes=nb)
    ar.check()
    for q in range(3):                       # slab columns of a sum that was not requested stay NaN, the others are all written
        col = scratch[:, q * width:(q + 1) * width]
        assert bool(torch.isnan(col).all()) if not (mask >> q) & 1 else bool(torch.isfinite(col).all()), ("slab", q, mask)
    assert all_equal(dmod[:, 2 * width:], 7.0)
    if not mask & 1:
        assert all_equal(dmod[:, :width], 7.0)
    if not mask & 2:
        assert all_equal(dmod[:, width:2 * width], 7.0)
    if not mask & 4:
        assert all_equal(dw, 7.0)
    return {"dx": dx.clone(), "dshift": dmod[:, :width].clone(), "dscale": dmod[:, width:2 * width].clone(), "dweight": dw.clone()}


def check_one_ln_backward(lib, device, before, B, rpb, width, cfg, ncu, seed, eps=1e-6):
    x, w, mod, dh, dx_in = lnb_inputs(B, rpb, width, cfg["dh_f32"], seed, device)
    w_, mod_ = (w if cfg["weight"] else None), (mod if cfg["scale"] else None)
    run = lambda mode: run_ln_backward(lib, device, before, x, dh, cfg["dh_f32"], w_, mod_, eps, dx_in, mode, cfg["mask"], B, rpb, width, ncu)
    got = twice(lambda: run(cfg["dxin"]))
    if cfg["dxin"] == "inplace":
        assert bit_equal(got["dx"], run("in")["dx"]), "dx_out == dx_in differs from out of place"
    rpblk = ln_rows_per_block(rpb, B * rpb, ncu)
    sc_rows = mod[:, width:2 * width].double().repeat_interleave(rpb, 0) if cfg["scale"] else None
    ref = ref_ln_backward(x.double(), dh.double(), w.double() if cfg["weight"] else None, sc_rows, eps,
                          None if cfg["dxin"] == "none" else dx_in.double(), B, rpb, rpblk)
    case = f"width {width} B {B} rows/sample {rpb}"
    check_f32("layernorm_backward", case, "dx", got["dx"], *ref["dx"])
    for q, name in enumerate(("dshift", "dscale", "dweight")):
        if (cfg["mask"] >> q) & 1:
            check_f32("layernorm_backward", case, name, got[name], *ref[name])


def check_layernorm_backward(lib, device, widths=LNB_WIDTHS, Bs=LNB_BS, rpbs=LNB_RPBS, masks=LNB_MASKS, before=None):
    ncu = compute_units(device)
    for width in widths:
        for si, (B, rpb) in enumerate((B, rpb) for B in Bs for rpb in rpbs):
            for cfg in lnb_configs(si, masks):
                check_one_ln_backward(lib, device, before, B, rpb, width, cfg, ncu, 300 + width + 10 * rpb + B)


def check_layernorm_backward_training_partition(lib, device, before=None):
    """4 x 4224 rows of 1024 on the real CU count (256: 66 rows per block, 64 slots per sample); the fp64 reference runs on the device."""
    B, rpb, width = LNB_TRAIN
    cfg = dict(mask=7, dh_f32=0, weight=True, scale=True, dxin="in")
    check_one_ln_backward(lib, device, before, B, rpb, width, cfg, compute_units(device), 4224)


# ---- row-linear backward ------------------------------------------------------------------------------------------------------------
RLB_MS = (1, 2, 3, 4, 5, 8)
RLB_NS = (14, 70, 256, 257, 6144)          # 257: the smallest N with two workgroups; 6144: 24 slots
RLB_KS = (256, 512, 1024)                  # M = 8, K = 1024: the 64 KiB boundary and the shipped upsampler shape
RLB_ROWS = 256                             # ROWLINEAR_BWD_ROWS: output features per workgroup = rows of W per slab slot


def ref_rowlinear_backward(x, W, dy, silu_in):
    """dW[n, :] = sum_m dy[m, n] act(x[m, :]): MR additions and the product (MR = M rounded up to 1, 2, 4, 8; the extra rows add zeros).
    db: MR additions.  dx = act'(x) sum_n dy[m, n] W[n, k]: ceil(min(N, 256) / 4) additions in a wave's registers, 4 waves into LDS one
    after the other, ceil(slots / 4) + 2 in the slab reduce, the product, and act' (4 ulp for __expf on its two factors)."""
    M, K = x.shape
    N = W.shape[0]
    mr = 1 if M <= 1 else 2 if M <= 2 else 4 if M <= 4 else 8
    xa = silu64(x) if silu_in else x
    S = dy.abs().t() @ xa.abs()
    out = {"dW": (dy.t() @ xa, (mr + 1) * U * S + (4 * ULP * S if silu_in else 0.0)), "db": (dy.sum(0), mr * U * dy.abs().sum(0))}
    acc, S = dy @ W, dy.abs() @ W.abs()
    depth = ceil_div(min(N, RLB_ROWS), 4) + 4 + ceil_div(ceil_div(N, RLB_ROWS), 4) + 2 + 1
    if silu_in:
        s = torch.sigmoid(x)
        ds = dsilu64(x)
        out["dx"] = (ds * acc, (depth + 1) * U * S * ds.abs() + 4 * ULP * s * (1.0 + (x * (1.0 - s)).abs()) * S)
    else:
        out["dx"] = (acc, depth * U * S)
    return out


def rlb_inputs(M, N, K, device):
    g = torch.Generator().manual_seed(11 * N + K + M)
    x = torch.randn(M, K, generator=g)
    W = (torch.randn(N, K, generator=g) * 0.1).to(torch.bfloat16)
    dy = torch.randn(M, N, generator=g)
    return x.to(device), W.to(device), dy.to(device)


def check_one_rowlinear_backward(lib, device, before, M, N, K, mask, silu_in):
    """mask bit 0: dW, bit 1: db, bit 2: dx"""
    x, W, dy = rlb_inputs(M, N, K, device)
    nb = int(lib.dgs_dit_rowlinear_backward_scratch_bytes(M, N, K))
    assert nb == ceil_div(N, RLB_ROWS) * M * K * 4

    def run():
        ar = Arena(device)
        dW, db, dx = ar.take((N, K), torch.float32, 7.0), ar.take((N,), torch.float32, 7.0), ar.take((M, K), torch.float32, 7.0)
        scratch = ar.take((nb // 4,), torch.float32, float("nan"))
        call(lib, "dgs_dit_rowlinear_backward", _native.DgsDitRowLinearBackwardArgs, device, before, M=M, N=N, K=K, x=x,
             silu_input=silu_in, W=W, dy=dy, dW=dW if mask & 1 else None, db=db if mask & 2 else None, dx=dx if mask & 4 else None,
             scratch=scratch, scratch_bytes=nb)
        ar.check()
        for q, t in enumerate((dW, db, dx)):
            assert (mask >> q) & 1 or all_equal(t, 7.0), ("an output that was not requested was written", q)
        assert bool(torch.isfinite(scratch).all()) if mask & 4 else bool(torch.isnan(scratch).all())
        return {"dW": dW.clone(), "db": db.clone(), "dx": dx.clone()}
    got = twice(run)
    ref = ref_rowlinear_backward(x.double(), W.double(), dy.double(), silu_in)
    for q, name in enumerate(("dW", "db", "dx")):
        if (mask >> q) & 1:
            check_f32("rowlinear_backward", f"M {M} N {N} K {K}", name, got[name], *ref[name])


def rlb_configs(shape_idx, per_shape):
    """(mask, silu): the full subset with the SiLU alternating, then per_shape - 1 of the 16 (subset, SiLU) combinations, rotating."""
    yield 7, shape_idx % 2
    for j in range(per_shape - 1):
        c = (shape_idx * (per_shape - 1) + j) % 16
        yield c % 8, c // 8


def check_rowlinear_backward(lib, device, shapes=None, per_shape=5, before=None):
    if shapes is None:
        shapes = [(M, N, K) for N in RLB_NS for K in RLB_KS for M in RLB_MS]
    for si, (M, N, K) in enumerate(shapes):
        for mask, silu_in in rlb_configs(si, per_shape):
            check_one_rowlinear_backward(lib, device, before, M, N, K, mask, silu_in)


# ---- gate multiply ------------------------------------------------------------------------------------------------------------------
GATE_CASES = [(B, rows, width) for B in (1, 3) for rows in (64, 192) for width in (64, 192, 1024)]


def gate_inputs(B, rows, width, device):
    """dx, y and gate positive (same-signed column-sum terms), gate a column slice of [B, 6 width] that differs by O(1) between samples."""
    g = torch.Generator().manual_seed(B + rows + width)
    dx = 0.5 + torch.rand(B * rows, width, generator=g)
    y = (0.5 + torch.rand(B * rows, width, generator=g)).to(torch.bfloat16)
    mod = 0.5 + torch.rand(B, 6 * width, generator=g) + 1.5 * torch.arange(B, dtype=torch.float32)[:, None]
    return dx.to(device), y.to(device), mod.to(device)


def ref_gate_mul(dx, y, gate, B, rows):
    """dy = gate dx: one fp32 product in front of the bf16 rounding.  dgate = sum_t dx y: 16 additions in a thread (64 rows, every fourth),
    2 levels over the workgroup's four partial sums, ceil(slots / 4) + 2 in the slab reduce (slots = rows / 64), the product."""
    width = dx.shape[1]
    dy = gate.repeat_interleave(rows, 0) * dx
    t = dx * y
    depth = 16 + 2 + ceil_div(rows // 64, 4) + 2 + 1
    per_b = lambda v: v.reshape(B, rows, width).sum(1)
    return {"dy": (dy, U * dy.abs()), "dgate": (per_b(t), depth * U * per_b(t.abs()))}


def ref_gate_dbias(dy_rounded, B, rows):
    """dbias = the sum of dy AS ROUNDED over every row of every sample (exact terms): 16 + 2 + ceil(B slots / 4) + 2 additions."""
    depth = 16 + 2 + ceil_div(B * (rows // 64), 4) + 2
    return dy_rounded.sum(0), depth * U * dy_rounded.abs().sum(0)


def check_gate_mul(lib, device, cases=GATE_CASES, before=None):
    for B, rows, width in cases:
        dx, y, mod = gate_inputs(B, rows, width, device)
        gate = mod[:, 2 * width:3 * width]
        nb = int(lib.dgs_dit_gate_mul_scratch_bytes(B, rows, width))
        assert nb == B * (rows // 64) * 2 * width * 4
        ref = ref_gate_mul(dx.double(), y.double(), gate.double(), B, rows)
        for with_bias in (True, False):
            def run():
                ar = Arena(device)
                dy = ar.take((B * rows, width), torch.bfloat16, 7.0)
                dyT = ar.take((B, width, rows), torch.bfloat16, 7.0)
                dmod = ar.take((B, 6 * width), torch.float32, 7.0)
                dbias = ar.take((width,), torch.float32, 7.0)
                scratch = ar.take((nb // 4,), torch.float32, float("nan"))
                call(lib, "dgs_dit_gate_mul", _native.DgsDitGateMulArgs, device, before, B=B, rows=rows, width=width, dx=dx, y=y, gate=gate,
                     gate_stride=6 * width, dy=dy, dyT=dyT, dgate=dmod[:, 2 * width:], dbias=dbias if with_bias else None,
                     scratch=scratch, scratch_bytes=nb)
                ar.check()
                assert all_equal(dmod[:, :2 * width], 7.0) and all_equal(dmod[:, 3 * width:], 7.0), "dgate columns outside the slice were written"
                assert with_bias or all_equal(dbias, 7.0)
                return {"dy": dy.clone(), "dyT": dyT.clone(), "dgate": dmod[:, 2 * width:3 * width].clone(), "dbias": dbias.clone()}
            got = twice(run)
            case = f"B {B} rows {rows} width {width}"
            check_bf16("gate_mul", case, "dy bf16", got["dy"], *ref["dy"])
            assert bit_equal(got["dyT"], got["dy"].reshape(B, rows, width).transpose(1, 2).contiguous()), (case, "dyT is not the transpose of dy")
            check_f32("gate_mul", case, "dgate", got["dgate"], *ref["dgate"])
            if with_bias:
                check_f32("gate_mul", case, "dbias", got["dbias"], *ref_gate_dbias(got["dy"].double(), B, rows))


# ---- token scatter / gather ---------------------------------------------------------------------------------------------------------
TOKEN_NGS, TOKEN_LS, TOKEN_BS = (1, 2, 8), (18, 258, 264), (1, 3)


def check_tokens(lib, device, width, before=None):
    """dgs_dit_run_blocks with first == last (what DitEngine.run_blocks calls; here with the output and the workspace between guard bands):
    scatter into the padded rows, no block, gather back -- the output equals the input bit for bit and the padding rows of the residual
    stream, the first carve of the workspace, are still zero."""
    from dgs_amd.dit import DitEngine
    from oracle import dit_oracle as D
    for ng in TOKEN_NGS:
        cfg = D.Cfg(width=width, num_layers=1, n_gaussians=ng)
        eng = DitEngine(D.parity_state_dict(cfg, 0), width=width, num_layers=1, n_gaussians=ng, device=device, lib=lib)
        for L in TOKEN_LS:
            for B in TOKEN_BS:
                g = torch.Generator().manual_seed(L + B + ng)
                tokens = torch.randn(B, L, width, generator=g).to(device)
                cvec = torch.randn(B, width, generator=g).to(device)
                lpad = int(lib.dgs_dit_lpad(L))
                need = int(lib.dgs_dit_workspace_bytes_for_tokens(ctypes.byref(eng.model), B, L))
                assert need >= B * lpad * width * 4

                def run():
                    ar = Arena(device)
                    out = ar.take((B, L, width), torch.float32, 7.0)
                    ws = ar.take((need,), torch.uint8, 0)
                    a = _native.DgsDitRunBlocksArgs()
                    a.B, a.L, a.V, a.first, a.last = B, L, 0, 0, 0
                    a.tokens_in, a.cvec, a.tokens_out, a.workspace, a.workspace_bytes = tokens.data_ptr(), cvec.data_ptr(), out.data_ptr(), ws.data_ptr(), need
                    dev = torch.device(device)
                    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
                    if before:
                        before()
                    rc = lib.dgs_dit_run_blocks(ctypes.byref(eng.model), ctypes.byref(a), stream)
                    assert rc == 0, rc
                    ar.check()
                    xrows = ws[:B * lpad * width * 4].view(torch.float32).view(B, lpad, width)
                    assert all_equal(xrows[:, L:], 0.0), ("padding rows written", ng, L, B)
                    assert bit_equal(xrows[:, :L - ng], tokens[:, ng:]) and bit_equal(xrows[:, L - ng:L], tokens[:, :ng]), ("scatter", ng, L, B)
                    return {"out": out.clone()}
                assert bit_equal(twice(run)["out"], tokens), ("gather(scatter(tokens)) != tokens", ng, L, B)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def check_refusals(lib, device, before=None):
    """Shapes outside the launchers' limits return DGS_ERR_INVALID_ARGUMENT and leave every output untouched (nothing is enqueued)."""
    def untouched(ar, *outs):
        ar.check()
        for t in outs:
            assert all_equal(t, 7.0), "a refused call wrote to its output"

    for width in (1280, 320):
        rows = 8
        x = torch.randn(rows, width).to(device)
        ar = Arena(device)
        out = ar.take((rows, width), torch.float32, 7.0)
        call(lib, "dgs_dit_layernorm", _native.DgsDitLayerNormArgs, device, before, INVALID, rows=rows, width=width, x=x, mod_stride=0,
             rows_per_batch=0, eps=1e-6, out=out, out_f32=1)
        untouched(ar, out)
    for width in (768, 2048):
        rows = 16
        x, dh = torch.randn(rows, width).to(device), torch.randn(rows, width).to(device)
        nb = int(lib.dgs_dit_layernorm_backward_scratch_bytes(rows, width, rows))
        ar = Arena(device)
        dx, dmod, dw = ar.take((rows, width), torch.float32, 7.0), ar.take((1, 2 * width), torch.float32, 7.0), ar.take((width,), torch.float32, 7.0)
        scratch = ar.take((nb // 4,), torch.float32, 7.0)
        call(lib, "dgs_dit_layernorm_backward", _native.DgsDitLayerNormBackwardArgs, device, before, INVALID, rows=rows, width=width, x=x,
             dh=dh, dh_f32=1, mod_stride=2 * width, rows_per_batch=rows, eps=1e-6, dx_out=dx, dshift=dmod, dscale=dmod[:, width:],
             dweight=dw, scratch=scratch, scratch_bytes=nb)
        untouched(ar, dx, dmod, dw, scratch)
    for M, K in ((17, 256), (8, 4096), (16, 2048), (4, 8192)):          # M > 16; MR K 4 > 65536 for MR = 8, 16, 4
        N = 37
        x, W = torch.randn(M, K).to(device), torch.randn(N, K).to(torch.bfloat16).to(device)
        ar = Arena(device)
        out = ar.take((M, N), torch.float32, 7.0)
        call(lib, "dgs_dit_rowlinear", _native.DgsDitRowLinearArgs, device, before, INVALID, M=M, N=N, K=K, x=x, silu_input=0, W=W,
             silu_output=0, out=out)
        untouched(ar, out)
    for M, K in ((9, 256), (4, 2048)):
        N = 70
        x, W, dy = torch.randn(M, K).to(device), torch.randn(N, K).to(torch.bfloat16).to(device), torch.randn(M, N).to(device)
        nb = int(lib.dgs_dit_rowlinear_backward_scratch_bytes(M, N, K))
        ar = Arena(device)
        dW, db, dx = ar.take((N, K), torch.float32, 7.0), ar.take((N,), torch.float32, 7.0), ar.take((M, K), torch.float32, 7.0)
        scratch = ar.take((nb // 4,), torch.float32, 7.0)
        call(lib, "dgs_dit_rowlinear_backward", _native.DgsDitRowLinearBackwardArgs, device, before, INVALID, M=M, N=N, K=K, x=x,
             silu_input=0, W=W, dy=dy, dW=dW, db=db, dx=dx, scratch=scratch, scratch_bytes=nb)
        untouched(ar, dW, db, dx, scratch)


# ---- what the bars can tell apart (no kernel runs) ----------------------------------------------------------------------------------
def change_over_bar(mutant, ref, bar):
    """max over elements of |mutant - ref| / bar: a mutant is caught when this exceeds 2 (the bar is less than half the change)."""
    return float(((mutant - ref).abs() / bar.expand_as(ref).clamp_min(1e-300)).max())


def bf16_rule_catches(mutant, ref, bar):
    """Number of elements at which the mutant, rounded to nearest-even bf16, fails the bf16 rule (bf16_verdict) against ref."""
    bad, _, _ = bf16_verdict(mutant.float().to(torch.bfloat16), ref, bar.expand_as(ref))
    return int(bad.sum())


def one_pass_variance_fp32_layernorm(x, weight, shift, scale, rpb, eps):
    """ref_layernorm with the statistics of a one-pass fp32 kernel: var = E[x^2] - mean^2 evaluated in fp32."""
    xf = x.float()
    mean = xf.mean(-1, keepdim=True)
    var = ((xf * xf).mean(-1, keepdim=True) - mean * mean).clamp_min(0.0)
    y = (x - mean.double()) * (var.double() + eps).rsqrt()
    if weight is not None:
        y = y * weight
    if shift is not None:
        b = torch.arange(x.shape[0], device=x.device) // rpb
        y = y * (1.0 + scale[b]) + shift[b]
    return y
