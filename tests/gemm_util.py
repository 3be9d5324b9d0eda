"""The DiT GEMM kernels (csrc/dit_gemm.hip, csrc/dit_gemm_deep.hip) against fp64, one dispatch branch per case: case tables with the
plan each case claims, seeded inputs, fp64 references, guarded launches and the checks.  Shared by test_dit_gemm_emu.py (CPU emulator
build), test_dit_gemm_gpu.py (MI355X) and tools/dit_gemm_error.py.  Arena, bit_equal, twice and the bf16 rule come from rowkernel_util.

Harness (every case).  dgs_dit_gemm_plan must first equal the plan the table claims (family, tile width, waves, tail form, map2d,
tail_wgs > 0, nsplit, the 128-wide kernel's gemv_tail_rows): a case that drifts off its branch fails instead of testing another one.
`out`, `vt`, `aux` and the split-K scratch are views between two bands of 0xA5 bytes (checked bit for bit); `out` / `aux` get
ldo = N + 8 where the entry point takes a stride (not QKV, whose ldo is 2N/3 by contract, nor DGELU, whose `aux` is an input);
A and W get lda = ldw = K + 8 with NaN in the slack.  Outputs start as 7.0 (an in-place residual stream as the residual).  From the plan
follows which rows a launch writes (written_rows): whole tiles of a ring row, the live 32-row block of an MFMA item, live rows only of
GEMV items, the 32-row blocks with a live row on the 128-wide kernel.  Every other row, and the slack columns, must still hold the initial
bits; written padding rows must be finite and equal the reference like live rows.  Every call runs twice, bit-equal.  Mismatches are
counted per 32-row block x 64-column strip and the assertion names the worst one.

Exact regime: A integers in [-a, a], W and bias integers x 2^-6 (|w 2^6| <= wq, |bias 2^6| <= 32) with K a wq + 32 < 2^24 (asserted):
every partial sum in any order is an integer multiple of 2^-6 below 2^18 -- exact in fp32, so the result does not depend on the summation
order and fp32 torch equals fp64 torch bit for bit on the CPU (asserted on up to 256 rows of every case, the last live rows among them).
  F32                      bit-equal to the fp64 reference.
  BF16, aux, QKV k / v, q with q_scale 0.5:   exactly the round-to-nearest-even bf16; a = wq = 16 gives sums of 11 - 17 bits, and at
                           least half of the reference must not be bf16-representable (asserted).
  GATE_RESIDUAL            gate integers in [-8, 8], resid integers x 2^-6 below 2^10: (K a wq + 32) 8 + 2^10 < 2^24 (asserted), so
                           resid + gate v is exact with or without an FMA: bit-equal, in place and out of place.
  vt                       bit-equal to the transposed row-major output on written rows, initial bits elsewhere.
Inexact epilogues on exact pre-activations (GELU, DGELU, q with the production q_scale): an element must be the RNE bf16 of the fp64
reference unless the reference lies within the ZONE of a rounding midpoint (rowkernel_util.bf16_verdict); at most 0.5 % of a tensor may
take that exception, and the reference's own share of elements that close to a midpoint must be below 0.25 % (asserted on the CPU
side of the check, from the reference alone).  Zones (u = 2^-24; 1/2 ulp = u per multiply / add / FMA / constant conversion, 1 ulp = 2 u
for v_exp_f32 and v_rcp_f32), from epi_gelu_tanh / epi_dgelu_tanh of dit_gemm_epilogue.h as written:
  t = x fma(x x, c1, c0): c0 = -2 log2(e) sqrt(2/pi) costs 2 conversions + 1 multiply (3 u; -2 is exact), c1 = c0 0.044715 two more
      (5 u); x x: u; the fma adds two terms of one sign, so its relative error is at most max(5 u + u, 3 u) + u = 7 u; times x: 8 u.
      (The MFMA items of dit_gemm_deep.hip still use gelu_tanh_d: k (x + c x x x) through __expf = exp2(y log2(e)) and an IEEE division:
      9 u on the exponent, nothing larger elsewhere.  The zone takes 9 u so that one reference serves both.)
  e = exp2(t): 2 u + the argument's error through the exponential, |t| 9 u ln 2 <= 9 u |t|.
  d = 1 + e: relative (e / d) (2 u + 9 u |t|) + u.     r = rcp(d): + 2 u.     y = x r: + u.
  GELU zone   = |y| u (4 + s' (2 + 9 |t|)) + 2^-120,  s' = e / (1 + e)   (the floor: results below the fp32 normal range may flush).
  DGELU       sg = r: eps = u (3 + s' (2 + 9 |t|)).  P = fma(x x, 3 c, 1): <= 4 u.  T = x sg (1 - sg) K2 P, left to right: five multiplies,
              the subtraction and K2's conversion 7 u, P's 4 u -> |T| (eps + 11 u) + |x sg K2 P| sg eps (sg's error inside 1 - sg).
              dg = sg + T: sg eps + err T + u |dg|.    out = v dg: zone = |v| err dg + u |v dg| + 2^-120.
  q (production q_scale = fp32(0.125 log2 e), the reference multiplies by that fp32 value): one multiply: zone = u |ref|.
GELU / DGELU cases scale the operands down (a = 1, wq ~ sqrt(26680 / K)) so that at least half of the pre-activations have |x| < 3
(asserted).  With |x| < 3 on a 2^-6 grid x has at most 8 bits, so GELU's `aux` is then bf16-representable almost everywhere: that condition
and "half of the reference is not representable" exclude each other, and larger arguments put gelu(x) = x on exact rounding ties that fp64
cannot resolve.  GELU's aux is therefore checked bit for bit without the share condition; the same pack_bf2 store is exercised at full
share by GATE_RESIDUAL's aux and the BF16 output.  Where the result is exactly zero (x = 0, v = 0) or the zone is zero (the k features
beside pre-scaled q) the element must be the RNE bf16, no exception.

General regime (one case per family x tile x tail form): randn operands rounded to bf16, row 1 of A x 8, bias randn x 10^{-2..1}.
F32: |got - ref64| <= K 2^-23 sum_k |a_k w_k| per element (two units per addition: the MFMA's and v_dot2's internal rounding is not
specified); BF16: + half a bf16 step of the reference.  The ratio error / bar is recorded (RECORDS), never tuned to.

RECORDS: (case, regime, output and its type, plan, worst block, strip, error, bar, ratio, exception share); tools/dit_gemm_error.py writes them to
profiles/dit_gemm_parity.txt."""
import ctypes
import math
import os

import numpy as np
import torch

import rowkernel_util as R
from dgs_amd import _native
from rowkernel_util import Arena, bit_equal, bits, twice

U = R.U
SENTINEL = 7.0
FLOOR = 2.0 ** -120
EXCEPTION_CAP = R.EXCEPTION_CAP
RECORDS = []
F32, BF16, GELU, GATE, QKV, DGELU = _native.EPI_F32, _native.EPI_BF16, _native.EPI_GELU_BF16, _native.EPI_GATE_RESIDUAL, _native.EPI_QKV, _native.EPI_DGELU_BF16
EPI_NAME = {F32: "f32", BF16: "bf16", GELU: "gelu", GATE: "gate", QKV: "qkv", DGELU: "dgelu"}
AUTO, SIMPLE, SLICED, QUAD, S128 = _native.GEMM_AUTO, _native.GEMM_SIMPLE128, _native.GEMM_SLICED, _native.GEMM_QUAD, _native.GEMM_SLICED128
FAM_128, FAM_RING, FAM_RING128, FAM_SPLITK = 1, 2, 3, 4
TAIL_NONE, TAIL_GEMV, TAIL_MFMA, TAIL_RING = 0, 1, 2, 3
FAM_NAME = {1: "128-wide", 2: "ring", 3: "ring 128x128", 4: "split-K"}
TAIL_NAME = {0: "none", 1: "gemv", 2: "mfma", 3: "ring row"}
Q_PROD = float(np.float32(0.125 * math.log2(math.e)))      # what the C struct's float field holds for the denoiser's q_scale
INVALID = R.INVALID


def P(family, bn, waves, tail=TAIL_NONE, map2d=0, idle=False, nsplit=1, gemv_rows=0):
    """The plan a case claims; idle: tail_wgs > 0 (the side items run on workgroups of their own behind the tiles)."""
    return dict(family=family, bn=bn, waves=waves, tail_form=tail, map2d=map2d, idle=bool(idle), nsplit=nsplit, gemv_tail_rows=gemv_rows)


def C(name, M, N, K, epi, algo, plan, rpb=0, valid=0, **kw):
    c = dict(name=name, M=M, N=N, K=K, epi=epi, algo=algo, plan=plan, rpb=rpb, valid=valid, bias=True, vt=False, aux=False, inplace=True,
             qs=0.5, kpb=0, splitk=False, dense=False, gate_pad=0, regime="exact", cus=None, seed=0)
    unknown = set(kw) - set(c)
    assert not unknown, unknown
    c.update(kw)
    return c


def plan_text(p):
    return (f"{FAM_NAME[p['family']]} {p['bm']}x{p['bn']} {p['waves']}w items {p['full_items']} tail {TAIL_NAME[p['tail_form']]} {p['tail_items']}"
            f" tail_wgs {p['tail_wgs']} map2d {p['map2d']} nsplit {p['nsplit']}/{p['splits_per_batch']} gemv_rows {p['gemv_tail_rows']} grid {p['grid']}")


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def geometry(c):
    rpb = c["rpb"] or c["M"]
    valid = c["valid"] if 0 < c["valid"] < rpb else rpb
    kpb = c["kpb"] or c["K"]
    wide = c["epi"] in (F32, BF16, GELU, GATE) and not c["dense"]
    ldo = 2 * c["N"] // 3 if c["epi"] == QKV else c["N"] + (8 if wide else 0)
    return rpb, valid, kpb, ldo


def gemm_args(c, **ptr):
    """DgsDitGemmArgs of a case; ptr: tensors (or integers) for the pointer fields."""
    rpb, valid, kpb, ldo = geometry(c)
    a = _native.DgsDitGemmArgs()
    a.M, a.N, a.K, a.lda, a.ldw, a.ldo = c["M"], c["N"], c["K"], kpb + 8, kpb + 8, ldo
    a.epilogue, a.algo, a.rows_per_batch, a.valid_rows = c["epi"], c["algo"], c["rpb"], c["valid"]
    a.q_scale = Q_PROD if c["qs"] == "prod" else c["qs"]
    if c["kpb"]:
        a.k_per_batch, a.a_batch_stride, a.w_batch_stride = kpb, c["M"] * (kpb + 8), c["N"] * (kpb + 8)
    a.gate_stride = c["N"] + c["gate_pad"]
    for k, v in ptr.items():
        if v is not None:
            setattr(a, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return a


def plan_of(lib, c, expect=0):
    """dgs_dit_gemm_plan of the case (launches nothing: the pointers only have to be non-null where the dispatch looks at them)."""
    d = 64
    a = gemm_args(c, A=d, W=d, out=d, bias=d if c["bias"] else None, gate=d if c["epi"] == GATE else None,
                  vt=d if c["epi"] == QKV or c["vt"] else None, aux=d if c["epi"] == DGELU or c["aux"] else None, splitk_ws=d if c["splitk"] else None)
    p = _native.DgsDitGemmPlan()
    rc = lib.dgs_dit_gemm_plan(ctypes.byref(a), ctypes.byref(p))
    assert rc == expect, (c["name"], "dgs_dit_gemm_plan", rc)
    return {n: int(getattr(p, n)) for n, _ in p._fields_}


def claim_of(p):
    return P(p["family"], p["bn"], p["waves"], p["tail_form"], p["map2d"], p["tail_wgs"] > 0, p["nsplit"], p["gemv_tail_rows"])


def assert_plan(lib, c):
    p = plan_of(lib, c)
    assert claim_of(p) == c["plan"], (c["name"], "runs", plan_text(p), "but its table entry claims", c["plan"])
    return p


def written_rows(c, p):
    """bool [M]: the rows a launch with this plan writes (module docstring)."""
    rpb, valid, _, _ = geometry(c)
    w = torch.zeros(rpb, dtype=torch.bool)
    if p["family"] == FAM_128:
        w[:R.ceil_div(valid, 32) * 32] = True
        if p["gemv_tail_rows"]:
            r0 = (R.ceil_div(valid, 128) - 1) * 128
            w[r0:] = False
            w[r0:valid] = True
    elif p["family"] == FAM_SPLITK:
        w[:] = True
    else:
        bm = p["bm"]
        for i in range(rpb // bm):
            left = valid - i * bm
            live = (left + 31) // 32 if left > 0 else 0
            if live > 1 or (live == 1 and p["tail_form"] == TAIL_RING):
                w[i * bm:(i + 1) * bm] = True
            elif live == 1 and p["tail_form"] == TAIL_GEMV:
                w[i * bm:valid] = True
            elif live == 1 and p["tail_form"] == TAIL_MFMA:
                w[i * bm:i * bm + 32] = True
    return w.repeat(c["M"] // rpb)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def exact_ranges(c):
    """(a, wq, boost): |A| <= a, |W 2^6| <= wq (x boost on every 8th output column), with the exactness condition asserted."""
    K = c["K"]
    if c["epi"] in (GELU, DGELU):
        a, wq, boost = 1, max(1, round(math.sqrt(26680.0 / K))), 1
    else:
        a, wq, boost = 16, 16, 1
    top = K * a * wq * boost + 32
    if c["epi"] == GATE:
        top = top * 8 + 1024
    assert top < 2 ** 24, (c["name"], "partial sums are not exact in fp32", top)
    return a, wq, boost


def inputs(c):
    """CPU tensors of a case: A [nb, M, kpb], W [nb, N, kpb] (values exactly bf16), bias, gate, resid, u (DGELU's aux input)."""
    rpb, valid, kpb, ldo = geometry(c)
    M, N, K = c["M"], c["N"], c["K"]
    nb = K // kpb
    g = torch.Generator().manual_seed(1000 + c["seed"] + M + 3 * N + 7 * K + 11 * c["epi"])
    d = {}
    if c["regime"] == "exact":
        a, wq, boost = exact_ranges(c)
        d["A"] = torch.randint(-a, a + 1, (nb, M, kpb), generator=g).float()
        W = torch.randint(-wq, wq + 1, (nb, N, kpb), generator=g).float()
        if boost > 1:
            W[:, 7::8] *= boost
        d["W"] = W / 64
        d["bias"] = torch.randint(-32, 33, (N,), generator=g).float() / 64
        d["gate"] = torch.randint(-8, 9, (M // rpb, N), generator=g).float()
        d["resid"] = torch.randint(-1023, 1024, (M, N), generator=g).float() / 64
    else:
        A = torch.randn(nb, M, kpb, generator=g)
        A[:, 1] *= 8
        d["A"] = A.bfloat16().float()
        d["W"] = (torch.randn(nb, N, kpb, generator=g) * 0.2).bfloat16().float()
        d["bias"] = torch.randn(N, generator=g) * 10.0 ** torch.randint(-2, 2, (N,), generator=g).float()
        d["gate"] = torch.randn(M // rpb, N, generator=g)
        d["resid"] = torch.randn(M, N, generator=g)
    d["u"] = torch.randint(-96, 97, (M, N), generator=g).float() / 32          # DGELU's saved pre-activation, |u| <= 3: exactly bf16 (8 bits)
    if not c["bias"]:
        d["bias"] = None
    assert bool((d["A"].bfloat16().float() == d["A"]).all()) and bool((d["W"].bfloat16().float() == d["W"]).all())
    return d


def check_reference_is_exact(c, d):
    """The exact regime's premise, on the reference alone: fp32 and fp64 torch give the same bits on the CPU (up to 256 rows per case:
    the first 128 and the 128 around the last live row of the first sample)."""
    rpb, valid, kpb, _ = geometry(c)
    rows = sorted(set(range(min(128, c["M"]))) | set(range(max(0, valid - 96), min(c["M"], valid + 32))))
    A, W = d["A"][:, rows], d["W"]
    v32 = sum(A[b] @ W[b].t() for b in range(A.shape[0]))
    v64 = sum(A[b].double() @ W[b].double().t() for b in range(A.shape[0]))
    if d["bias"] is not None:
        v32, v64 = v32 + d["bias"], v64 + d["bias"].double()
    assert bool((v32.double() == v64).all()), (c["name"], "the fp32 and fp64 references differ: the inputs are not exact")


# ---- references (fp64, on the device of the run) -------------------------------------------------------------------------------------
K_TANH, C_TANH = math.sqrt(2.0 / math.pi), 0.044715


def gelu_parts(x):
    w = K_TANH * (x + C_TANH * x ** 3)
    sg = torch.sigmoid(2 * w)
    return sg, torch.sigmoid(-2 * w), (2 * math.log2(math.e) * w).abs()       # sigmoid(2u), s' = 1 - it, |t|


def ref_gelu(x):
    """(y, zone): gelu_tanh in fp64 and the fp32 error zone of epi_gelu_tanh (module docstring)."""
    sg, s1, t = gelu_parts(x)
    y = x * sg
    return y, torch.where(y == 0, torch.zeros_like(y), y.abs() * U * (4 + s1 * (2 + 9 * t)) + FLOOR)


def ref_dgelu(v, x):
    """(v gelu_tanh'(x), zone of epi_dgelu_tanh and the product)."""
    sg, s1, t = gelu_parts(x)
    eps = U * (3 + s1 * (2 + 9 * t))
    k2 = 2 * K_TANH
    pp = 1 + 3 * C_TANH * x * x
    T = x * sg * s1 * k2 * pp
    err_t = T.abs() * (eps + 11 * U) + (x * sg * k2 * pp).abs() * sg * eps
    dg = sg + T
    err = sg * eps + err_t + U * dg.abs()
    return v * dg, torch.where(v == 0, torch.zeros_like(v), v.abs() * err + U * (v * dg).abs() + FLOOR)


def reference(c, dd):
    """fp64 [M, N] pre-epilogue values v (and sum |a w| in the general regime) from device tensors."""
    A, W = dd["A"].double(), dd["W"].double()
    v = sum(A[b] @ W[b].t() for b in range(A.shape[0]))
    absdot = sum(A[b].abs() @ W[b].abs().t() for b in range(A.shape[0])) if c["regime"] != "exact" else None
    if dd["bias"] is not None:
        v = v + dd["bias"].double()
    return v, absdot


def rne_bf16(x64):
    return x64.float().bfloat16()


def not_bf16_share(x64):
    return float((rne_bf16(x64).double() != x64).double().mean())


def midpoint_share(ref, zone):
    """Share of a reference tensor that lies within `zone` of a bf16 rounding midpoint."""
    lo, hi = R.bf16_neighbours(ref)
    return float(((((lo + hi) / 2 - ref).abs() <= zone) & (zone > 0)).double().mean())


# ---- the checks ----------------------------------------------------------------------------------------------------------------------
def worst_block(bad, weight=None):
    """(text, block, strip) of the 32-row block x 64-column strip with the most wrong elements (or the largest weight)."""
    M, N = bad.shape
    sw = 64 if N % 64 == 0 else N
    t = (weight if weight is not None else bad.double()).reshape(M // 32, 32, N // sw, sw)
    per = t.amax((1, 3)) if weight is not None else t.sum((1, 3))
    i = int(per.argmax())
    blk, strip = i // per.shape[1], i % per.shape[1]
    return f"32-row block {blk} (rows {32 * blk}..{32 * blk + 31}), 64-column strip {strip} (columns {sw * strip}..{sw * strip + sw - 1})", blk, strip


def _fail(c, name, bad, got, ref, plan):
    text, blk, strip = worst_block(bad)
    idx = bad.nonzero()
    blocks = int(bad.reshape(bad.shape[0] // 32, 32, -1).any(2).any(1).sum())
    m, n = (int(x) for x in idx[0])
    return (f"{c['name']} [{plan_text(plan)}] {name}: {int(bad.sum())} wrong elements in {blocks} 32-row blocks; worst: {text}; "
            f"first at [{m}, {n}]: got {float(got[m, n])!r}, reference {float(ref[m, n])!r}")


def check_output(c, plan, name, got, init, want, written, rule, zone=None, bar=None):
    """got / init [M, ld] (the launch's result and what the buffer held before), want fp64 [M, N], written bool [M].
    rule: 'bits' (got == want cast to got's type, bit for bit), 'zone' (bf16 rule with an error zone), 'bar' (general regime)."""
    M, N = want.shape
    w = written.to(got.device)
    untouched = bits(got) == bits(init)
    keep = untouched[:, N:].all() and untouched[~w].all()
    if not bool(keep):
        bad = ~untouched[:, :N] & ~w[:, None]
        where = worst_block(bad)[0] if bool(bad.any()) else "the slack columns behind N"
        raise AssertionError(f"{c['name']} [{plan_text(plan)}] {name}: rows the plan does not write were written: {where}")
    g = got[:, :N]
    assert bool(torch.isfinite(g.float()[w]).all()), (c["name"], name, "non-finite value in a written row")
    share, err, barv, ratio = None, 0.0, 0.0, 0.0
    if rule == "bits":
        exp = want.to(got.dtype) if got.dtype == torch.float32 else rne_bf16(want)
        bad = (bits(g) != bits(exp)) & w[:, None]
        diff = (g.double() - want).abs() * w[:, None]
        err, ratio = float(diff.max()), float(bad.any())
        text, blk, strip = worst_block(bad)
    elif rule == "zone":
        wrong, took, rat = R.bf16_verdict(g, want, zone)
        strict = zone == 0                                       # no exception there: a tie goes to the even neighbour
        wrong = torch.where(strict, bits(g) != bits(rne_bf16(want)), wrong)
        took = took & ~strict
        bad = wrong & w[:, None]
        share = float((took & w[:, None]).double().sum() / max(1, int(w.sum()) * N))
        text, blk, strip = worst_block(bad, rat * w[:, None])
        i = int((rat * w[:, None]).argmax())
        err, barv, ratio = float((g.double() - want).abs().flatten()[i]), float(zone.flatten()[i]), float(rat.flatten()[i])
    else:
        if got.dtype == torch.bfloat16:
            lo, hi = R.bf16_neighbours(want)
            bar = bar + (hi - lo).abs() / 2
        diff = (g.double() - want).abs()
        rat = torch.where(diff == 0, torch.zeros_like(diff), diff / bar.clamp_min(1e-300)) * w[:, None]
        bad = rat > 1.0
        text, blk, strip = worst_block(bad, rat)
        i = int(rat.argmax())
        err, barv, ratio = float(diff.flatten()[i]), float(bar.flatten()[i]), float(rat.flatten()[i])
    RECORDS.append((c["name"], c["regime"], name + (" f32" if got.dtype == torch.float32 else " bf16"), plan_text(plan), blk, strip, err, barv, ratio, share))
    assert not bool(bad.any()), _fail(c, name, bad, g.double(), want, plan)
    if share is not None:
        assert share <= EXCEPTION_CAP, (c["name"], name, "share of either-neighbour exceptions", share, "cap", EXCEPTION_CAP)


def check_vt(c, plan, vt, vt_init, rowmajor, written, cols):
    """vt [B, F, rpb] against the row-major bf16 output's columns `cols` (F of them): bit-equal on written rows, initial bits elsewhere."""
    B, F, rpb = vt.shape
    w = written.to(vt.device).reshape(B, 1, rpb)
    exp = rowmajor[:, cols].reshape(B, rpb, F).transpose(1, 2)
    okw = (bits(vt) == bits(exp.contiguous())) | ~w
    oku = (bits(vt) == bits(vt_init)) | w
    bad = ~(okw & oku)
    if bool(bad.any()):
        b, f, t = (int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"{c['name']} [{plan_text(plan)}] vt: {int(bad.sum())} wrong elements; first: sample {b}, feature {f} (64-column strip {f // 64}), "
                             f"token {t} (32-row block {t // 32}): got {float(vt[b, f, t])}, row-major {float(exp[b, f, t])}, written row: {bool(w[b, 0, t])}")
    RECORDS.append((c["name"], c["regime"], "vt bf16", plan_text(plan), 0, 0, 0.0, 0.0, 0.0, None))


def _padded(t, device):
    """[nb, rows, k] -> bf16 device tensor [nb, rows, k + 8] with NaN in the slack columns."""
    nb, rows, k = t.shape
    p = torch.full((nb, rows, k + 8), float("nan"), dtype=torch.bfloat16, device=device)
    p[:, :, :k] = t.to(device).bfloat16()
    return p


def run_case(lib, device, c, before=None):
    """One case: plan assertion, two guarded launches, every output against its reference."""
    device = torch.device(device)
    M, N, epi = c["M"], c["N"], c["epi"]
    rpb, valid, kpb, ldo = geometry(c)
    B = M // rpb
    plan = assert_plan(lib, c)
    written = written_rows(c, plan)
    d = inputs(c)
    exact = c["regime"] == "exact"
    if exact:
        check_reference_is_exact(c, d)
    dd = {k: (v.to(device) if v is not None else None) for k, v in d.items()}
    A, W = _padded(d["A"], device), _padded(d["W"], device)
    gate = None
    if epi == GATE:
        gate = torch.full((B, N + c["gate_pad"]), float("nan"), device=device)
        gate[:, :N] = dd["gate"]
    out_dtype = torch.float32 if epi in (F32, GATE) else torch.bfloat16
    u_in = None
    if epi == DGELU:
        u_in = dd["u"].bfloat16().contiguous()
    inplace = epi == GATE and c["inplace"]
    resid = dd["resid"].contiguous() if epi == GATE else None
    if epi == GATE and not inplace:                      # out of place: a residual stream with the output's stride, NaN in the slack
        rs = torch.full((M, ldo), float("nan"), device=device)
        rs[:, :N] = resid
        resid = rs
    nsk = int(lib.dgs_dit_gemm_splitk_bytes(M, N, c["K"], kpb)) if c["splitk"] else 0
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream) if device.type == "cuda" else None
    inits = {}

    def run():
        ar = Arena(device)
        bufs = {"out": ar.take((M, ldo), out_dtype, SENTINEL)}
        if inplace:
            bufs["out"][:, :N] = resid
        if epi == QKV:
            bufs["vt"] = ar.take((B, N // 3, rpb), torch.bfloat16, SENTINEL)
        elif c["vt"]:
            bufs["vt"] = ar.take((B, N, rpb), torch.bfloat16, SENTINEL)
        if c["aux"] and epi in (GELU, GATE):
            bufs["aux"] = ar.take((M, ldo), torch.bfloat16, SENTINEL)
        ws = ar.take((max(nsk, 16) // 4,), torch.float32, float("nan")) if c["splitk"] else None
        inits.update({k: v.clone() for k, v in bufs.items()})
        a = gemm_args(c, A=A, W=W, out=bufs["out"], bias=dd["bias"], gate=gate, vt=bufs.get("vt"), aux=u_in if epi == DGELU else bufs.get("aux"),
                      resid=None if inplace else resid, splitk_ws=ws if nsk else None)
        if before:
            before()
        rc = lib.dgs_dit_gemm(ctypes.byref(a), stream)
        assert rc == 0, (c["name"], "dgs_dit_gemm", rc)
        ar.check()
        return {k: v.clone() for k, v in bufs.items()}

    got = twice(run)
    v, absdot = reference(c, dd)
    bar = None if exact else c["K"] * 2.0 ** -23 * absdot
    out, init = got["out"], inits["out"]

    def bf16_out(name, g, i, want, zone=None):
        if not exact:
            check_output(c, plan, name, g, i, want, written, "bar", bar=bar if zone is None else bar + zone)
        elif zone is None:
            assert not_bf16_share(want) >= 0.5, (c["name"], name, "the reference does not exercise the bf16 rounding", not_bf16_share(want))
            check_output(c, plan, name, g, i, want, written, "bits")
        else:
            own = midpoint_share(want, zone)
            assert own < EXCEPTION_CAP / 2, (c["name"], name, "the reference's own share of elements inside the zone", own)
            check_output(c, plan, name, g, i, want, written, "zone", zone=zone)

    if epi == F32:
        check_output(c, plan, "out", out, init, v, written, "bits" if exact else "bar", bar=bar)
    elif epi == BF16:
        bf16_out("out", out, init, v)
    elif epi == GATE:
        r = dd["resid"].double()
        g = dd["gate"].double().repeat_interleave(rpb, 0)
        gbar = None if exact else bar * g.abs() + 2 * U * ((g * v).abs() + r.abs())       # the product's and the sum's roundings
        check_output(c, plan, "out", out, init, r + g * v, written, "bits" if exact else "bar", bar=gbar)
        if "aux" in got:
            bf16_out("aux", got["aux"], inits["aux"], v)
    elif epi == GELU:
        if exact:
            assert float((v.abs() < 3).double().mean()) >= 0.5, (c["name"], "fewer than half of the pre-activations have |x| < 3")
        y, zone = ref_gelu(v)
        if exact:
            bf16_out("out", out, init, y, zone)
        else:                                                # the pre-activation's error through a slope of at most 1.13
            check_output(c, plan, "out", out, init, y, written, "bar", bar=1.13 * bar + zone)
        if "aux" in got:
            if exact:
                check_output(c, plan, "aux", got["aux"], inits["aux"], v, written, "bits")
            else:
                check_output(c, plan, "aux", got["aux"], inits["aux"], v, written, "bar", bar=bar)
    elif epi == DGELU:
        y, zone = ref_dgelu(v, dd["u"].double())
        if exact:
            bf16_out("out", out, init, y, zone)
        else:
            check_output(c, plan, "out", out, init, y, written, "bar", bar=1.13 * bar + zone)
    elif epi == QKV:
        third = N // 3
        qs = float(np.float32(Q_PROD)) if c["qs"] == "prod" else c["qs"]
        qk = torch.cat([v[:, :third] * qs, v[:, third:2 * third]], 1)
        if c["qs"] == "prod":
            zone = torch.cat([U * qk[:, :third].abs(), torch.zeros_like(qk[:, third:])], 1)
            if exact:
                assert not_bf16_share(qk[:, third:]) >= 0.5
                bf16_out("out", out, init, qk, zone)
            else:
                check_output(c, plan, "out", out, init, qk, written, "bar", bar=bar[:, :2 * third] + zone)
        elif exact:
            bf16_out("out", out, init, qk)
        else:
            check_output(c, plan, "out", out, init, qk, written, "bar", bar=bar[:, :2 * third])
        vfeat = v[:, 2 * third:]
        vt_rm = got["vt"].transpose(1, 2).reshape(M, third)
        init_rm = inits["vt"].transpose(1, 2).reshape(M, third)
        if exact:
            assert not_bf16_share(vfeat) >= 0.5
            check_output(c, plan, "v (from vt)", vt_rm, init_rm, vfeat, written, "bits")
        else:
            check_output(c, plan, "v (from vt)", vt_rm, init_rm, vfeat, written, "bar", bar=bar[:, 2 * third:])
    if c["vt"] and epi != QKV:
        check_vt(c, plan, got["vt"], inits["vt"], out[:, :N], written, slice(0, N))
    return plan


def check_refusals(lib, device, before=None):
    """Every DGS_ERR_INVALID_ARGUMENT condition of gemm_dispatch, of launch_sliced_gemm (QUAD on the 192-wide QKV tile) and of the
    plan entry point, from dgs_dit_gemm and from dgs_dit_gemm_plan; the outputs and their guards stay untouched.  Two conditions cannot
    be reached through the C ABI and have no case: launch_sliced's `rows_external` without GEMV rows (dgs_dit_layernorm_gemm asks
    gemm_leaves_rows_out, the same condition, before it takes that form; check_layernorm_gemm covers the fall-back to two launches) and
    launch_splitk_gemm's own argument test (gemm_dispatch tests the same fields before it calls it; a shape splitk_plan turns down runs
    the single-pass kernel: the last case below)."""
    device = torch.device(device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream) if device.type == "cuda" else None
    ar = Arena(device)
    out = ar.take((256, 392), torch.float32, SENTINEL)
    vt = ar.take((1, 384, 256), torch.bfloat16, SENTINEL)
    aux = ar.take((256, 392), torch.bfloat16, SENTINEL)
    ws = ar.take((4 * 256 * 384,), torch.float32, SENTINEL)
    A = torch.zeros(256, 264, dtype=torch.bfloat16, device=device)
    W = torch.zeros(384, 264, dtype=torch.bfloat16, device=device)
    gate = torch.zeros(1, 384, device=device)

    def args(**f):
        a = _native.DgsDitGemmArgs()
        a.M, a.N, a.K, a.lda, a.ldw, a.ldo, a.epilogue = 256, 384, 256, 264, 264, 392, F32
        a.A, a.W, a.out = A.data_ptr(), W.data_ptr(), out.data_ptr()
        for k, v in f.items():
            setattr(a, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
        return a

    qkv = dict(epilogue=QKV, rows_per_batch=256, vt=vt, ldo=256)
    refused = [("no arguments", None), ("M = 0", args(M=0)), ("N < 0", args(N=-128)), ("K = 0", args(K=0)), ("M % 128", args(M=192)), ("N % 64", args(N=96)),
               ("K % 64", args(K=96)), ("A missing", args(A=None)), ("W missing", args(W=None)), ("out missing", args(out=None)), ("lda % 8", args(lda=260)),
               ("ldw % 8", args(ldw=260)), ("lda < K", args(lda=128)), ("ldw < K", args(ldw=128)), ("k_per_batch % 64", args(k_per_batch=96)),
               ("K % k_per_batch", args(k_per_batch=192)), ("gate missing", args(epilogue=GATE, rows_per_batch=256)),
               ("gate without rows_per_batch", args(epilogue=GATE, gate=gate)), ("QKV without vt", args(**dict(qkv, vt=None))),
               ("QKV N % 3", args(**dict(qkv, N=256))), ("QKV (N / 3) % 128", args(**dict(qkv, N=192))), ("DGELU without aux", args(epilogue=DGELU)),
               ("vt without rows_per_batch", args(epilogue=BF16, vt=vt)), ("QKV without rows_per_batch", args(**dict(qkv, rows_per_batch=0))),
               ("rows_per_batch % 128", args(rows_per_batch=64)), ("M % rows_per_batch", args(M=384, rows_per_batch=256)),
               ("unknown epilogue", args(epilogue=9)), ("unknown epilogue on the ring", args(epilogue=9, algo=SLICED)),
               ("unknown epilogue on the 128 x 128 ring", args(epilogue=9, algo=S128))]
    # QUAD has no 192-wide form: refused where QKV gets that tile (MI355X: 20 x 8 tiles; the emulator at DGS_EMU_CUS=8: 1 x 8).  The
    # operands here are smaller than this shape: the call is made only where the library says it takes the 192-wide tile
    for M192, rpb192 in ((5120, 2560), (256, 256)):
        a = args(**dict(qkv, M=M192, N=1536, K=128, rows_per_batch=rpb192, ldo=1024, algo=SLICED))
        if lib.dgs_dit_gemm_sliced_tile(ctypes.byref(a)) == 192:
            a.algo = QUAD
            refused.append(("QUAD on the 192-wide QKV tile", a))
            break
    else:
        raise AssertionError("no shape reaches the 192-wide QKV tile on this device")
    for text, a in refused:
        ref = ctypes.byref(a) if a is not None else None
        if before:
            before()
        assert lib.dgs_dit_gemm(ref, stream) == INVALID, (text, "dgs_dit_gemm accepted it")
        assert lib.dgs_dit_gemm_plan(ref, ctypes.byref(_native.DgsDitGemmPlan())) == INVALID, (text, "dgs_dit_gemm_plan accepted it")
    assert lib.dgs_dit_gemm_plan(ctypes.byref(args()), None) == INVALID
    # not refusals: QKV asks for the 128 x 128 ring form (sliced128_eligible turns it down) and runs the 128-wide kernel; a split-K scratch
    # on a shape splitk_plan turns down runs the single-pass kernel
    q = C("qkv s128", 256, 768, 256, QKV, S128, None, rpb=256)
    assert plan_of(lib, q)["family"] == FAM_128
    s = C("split-K refused", 256, 256, 256, F32, AUTO, None, splitk=True, bias=False)
    assert lib.dgs_dit_gemm_splitk_bytes(256, 256, 256, 0) == 0 and plan_of(lib, s)["family"] != FAM_SPLITK
    ar.check()
    for t in (out, vt, aux, ws):
        assert R.all_equal(t.float(), SENTINEL), "a refused call wrote to an output"


def check_layernorm_gemm(lib, device, before=None, width=512, B=2, rpb=512, valid=258):
    """dgs_dit_layernorm_gemm in the form that shares rows (the learned tokens' output rows come from the first workgroups of the LayerNorm
    launch), on the ring kernel's 128-wide tile -- a shape that takes that form at any CU count.  (1) seeded random data: every output bit for
    bit what dgs_dit_layernorm + dgs_dit_gemm give.  (2) the GEMM part against fp64: scale = -1 makes the modulated LayerNorm output the
    shift vector exactly (integers), W and bias are on the 2^-6 grid, so the exact regime's rules apply to the pair's outputs.
    Outputs here are DitOps' zero-filled tensors (no guard bands: the plain launches these are compared with have them in run_case)."""
    from dgs_amd.dit import DitOps
    ops = DitOps(lib)
    dev = torch.device(device)
    M = B * rpb
    for epi, N in ((QKV, 1536), (GELU, 512)):
        g = torch.Generator().manual_seed(width + N + epi)
        c = C(f"layernorm_gemm {EPI_NAME[epi]}", M, N, width, epi, SLICED, P(FAM_RING, 128, 8, TAIL_GEMV, idle=True), rpb=rpb, valid=valid, dense=True)
        plan = plan_of(lib, c)
        assert plan["family"] == FAM_RING and plan["tail_form"] == TAIL_GEMV, plan_text(plan)
        written = written_rows(c, plan)
        wq = 16 if epi == QKV else 2                       # GELU: |shift| <= 3, |w 2^6| <= 2 at width 512: pre-activations of about 1
        for exact in (False, True):
            x = torch.randn(M, width, generator=g).to(dev)
            if exact:
                shift = torch.randint(-16 if epi == QKV else -3, (17 if epi == QKV else 4), (B, width), generator=g).float()
                mod = torch.cat([shift, -torch.ones(B, width)], 1).to(dev)
                W = (torch.randint(-wq, wq + 1, (N, width), generator=g).float() / 64).bfloat16().to(dev)
                bias = (torch.randint(-32, 33, (N,), generator=g).float() / 64).to(dev)
            else:
                mod = (torch.randn(B, 2 * width, generator=g) * 0.3).to(dev)
                W = (torch.randn(N, width, generator=g) * 0.05).bfloat16().to(dev)
                bias = torch.randn(N, generator=g).to(dev)
            shift_d, scale_d = mod[:, :width], mod[:, width:]
            if before:
                before()
            h_ref = ops.layernorm(x, shift=shift_d, scale=scale_d, rows_per_batch=rpb)
            if before:
                before()
            ref = ops.gemm(h_ref, W, bias, epi, rows_per_batch=rpb, valid_rows=valid, algo=SLICED, q_scale=0.5)
            if before:
                before()
            got = ops.layernorm_gemm(x, shift_d, scale_d, W, bias, epi, rpb, valid, algo=SLICED, q_scale=0.5)
            assert ops.last_pair_shared_rows, (c["name"], "the pair did not take the shared-rows form")
            ref = ref if epi == QKV else (ref,)
            assert bit_equal(got[0], h_ref), (c["name"], "LayerNorm output differs from the plain launch")
            for k, (a, b) in enumerate(zip(got[1:], ref)):
                assert bit_equal(a, b), (c["name"], "output", k, "differs from the two plain launches", "exact" if exact else "random")
            if exact:
                hv = h_ref.double()
                assert bool((hv == shift_d.double().repeat_interleave(rpb, 0)).all()), "scale = -1 did not give the shift vector"
                v = hv @ W.double().t() + bias.double()
                zero = torch.zeros_like(got[1])
                if epi == QKV:
                    third = N // 3
                    qk = torch.cat([v[:, :third] * 0.5, v[:, third:2 * third]], 1)
                    check_output(c, plan, "out", got[1], zero, qk, written, "bits")
                    check_output(c, plan, "v (from vt)", got[2].transpose(1, 2).reshape(M, third), zero[:, :third], v[:, 2 * third:], written, "bits")
                else:
                    assert float((v.abs() < 3).double().mean()) >= 0.5
                    y, zone = ref_gelu(v)
                    assert midpoint_share(y, zone) < EXCEPTION_CAP / 2
                    check_output(c, plan, "out", got[1], zero, y, written, "zone", zone=zone)


# ---- case tables ---------------------------------------------------------------------------------------------------------------------
def _tails(tag, algo, fam, bn, waves, idle_shape, busy_shape, ring_K, epis, busy_map2d=0):
    """The tail forms of one kernel form.  idle_shape / busy_shape = (rows per sample, samples, N): fewer full tiles than the chip has CUs
    (the items get workgroups of their own, tail_wgs > 0) / at least as many (the first tile workgroups take them).  One tile row of
    every sample holds the tail.  epis: the epilogues of the four item cases (the side items' own store paths)."""
    bm = 128 if fam == FAM_RING128 else 256
    out = []
    for (rpb, B, N), idle, (gK, live_g), live_m, (eg, em) in ((idle_shape, True, (512, 1), 3, epis[:2]), (busy_shape, False, (4096, 2), 32, epis[2:])):
        full = rpb - bm
        w = "idle" if idle else "busy"
        out.append(C(f"{tag} {w} gemv K{gK} live {live_g} {EPI_NAME[eg]}", rpb * B, N, gK, eg, algo, P(fam, bn, waves, TAIL_GEMV, map2d=0 if idle else busy_map2d, idle=idle), rpb=rpb,
                     valid=full + live_g, vt=eg in (BF16, GELU, DGELU), aux=eg in (GELU, GATE)))
        out.append(C(f"{tag} {w} mfma live {live_m} {EPI_NAME[em]}", rpb * B, N, 1024, em, algo, P(fam, bn, waves, TAIL_MFMA, map2d=0 if idle else busy_map2d, idle=idle), rpb=rpb,
                     valid=full + live_m, vt=em in (BF16, GELU, DGELU), aux=em in (GELU, GATE), inplace=False))
    rpb, B, N = idle_shape
    out.append(C(f"{tag} ring row K{ring_K}", rpb * B, N, ring_K, F32, algo, P(fam, bn, waves, TAIL_RING), rpb=rpb, valid=rpb - bm + 2))
    return out


R8, R4, R128N = dict(family=FAM_RING, bn=256, waves=8), dict(family=FAM_RING, bn=256, waves=4), dict(family=FAM_RING, bn=128, waves=8)
R192, RS = dict(family=FAM_RING, bn=192, waves=8), dict(family=FAM_RING128, bn=128, waves=8)
# section 3 of the issue: what the GPU table has to reach, as partial plans (test_dit_gemm_gpu.py::test_table_reaches_every_branch)
REQUIRED = [("ring 256x256 8 waves, map2d", dict(R8, map2d=1)), ("ring 256x256 8 waves, xcd order", dict(R8, map2d=0, tail_form=TAIL_NONE)),
            ("ring 256x256 4 waves, map2d", dict(R4, map2d=1)), ("ring 256x256 4 waves, xcd order", dict(R4, map2d=0, tail_form=TAIL_NONE)),
            ("ring 256x192, map2d", dict(R192, map2d=1)), ("ring 256x192, xcd order", dict(R192, map2d=0)), ("ring 256x128", R128N), ("ring 128x128", RS),
            ("128-wide, BN 128", dict(family=FAM_128, bn=128)), ("128-wide, BN 64", dict(family=FAM_128, bn=64)),
            ("128-wide, gemv_tail_rows", dict(family=FAM_128, gemv_tail_rows=1)), ("split-K", dict(family=FAM_SPLITK, nsplit=8))]
for _n, _f in (("256x256 8 waves", R8), ("256x256 4 waves", R4), ("256x128", R128N), ("128x128", RS)):
    for _t in (TAIL_GEMV, TAIL_MFMA):
        for _i in (True, False):
            REQUIRED.append((f"ring {_n}, {TAIL_NAME[_t]} items, " + ("idle CUs" if _i else "first workgroups"), dict(_f, tail_form=_t, idle=_i)))
    REQUIRED.append((f"ring {_n}, tail row on the ring", dict(_f, tail_form=TAIL_RING)))


def reaches(plan_claim, want):
    return all(plan_claim[k] == v for k, v in want.items())


def gpu_cases():
    """The MI355X table (256 CUs).  Shapes: the smallest that reach the branch; sliced_gemm_tile gives 256-wide tiles from 160 tiles on."""
    t = []
    # ring 256 x 256, 8 and 4 waves: 8 x 20 tiles (map2d), 10 x 16 (rows % 4: xcd order), 10 x 32 (more tiles than CUs); K = one trip of the
    # ring, 12 slabs, 8 trips
    for algo, waves, tag in ((SLICED, 8, "ring256"), (QUAD, 4, "quad256")):
        pl = lambda **kw: P(FAM_RING, 256, waves, **kw)
        t += [C(f"{tag} map2d K128 f32", 2048, 5120, 128, F32, algo, pl(map2d=1)),
              C(f"{tag} xcd K384 bf16+vt", 2560, 4096, 384, BF16, algo, pl(), rpb=2560, vt=True),
              C(f"{tag} 320 tiles K1024 f32", 2560, 8192, 1024, F32, algo, pl()),
              C(f"{tag} map2d K128 gelu+aux+vt", 2048, 5120, 128, GELU, algo, pl(map2d=1), rpb=1024, aux=True, vt=True),
              C(f"{tag} map2d K128 dgelu+vt", 2048, 5120, 128, DGELU, algo, pl(map2d=1), rpb=2048, vt=True),
              C(f"{tag} map2d K128 gate in place+aux", 2048, 5120, 128, GATE, algo, pl(map2d=1), rpb=1024, aux=True, gate_pad=5120 * 5),
              C(f"{tag} map2d K128 gate out of place, no bias", 2048, 5120, 128, GATE, algo, pl(map2d=1), rpb=1024, inplace=False, bias=False),
              C(f"{tag} xcd K128 qkv 256-wide", 2560, 5376, 128, QKV, algo, pl(), rpb=1280),
              C(f"{tag} general f32", 2048, 5120, 384, F32, algo, pl(map2d=1), regime="general"),
              C(f"{tag} general bf16", 2048, 5120, 384, BF16, algo, pl(map2d=1), regime="general")]
        t += _tails(tag, algo, FAM_RING, 256, waves, (2816, 1, 4096), (2304, 2, 4096), 384, (F32, BF16, GATE, GELU), busy_map2d=1)
        t += [C(f"{tag} general gemv items", 2816, 4096, 512, F32, algo, pl(tail=TAIL_GEMV, idle=True), rpb=2816, valid=2562, regime="general"),
              C(f"{tag} general mfma items", 2816, 4096, 1024, BF16, algo, pl(tail=TAIL_MFMA, idle=True), rpb=2816, valid=2570, regime="general")]
    t.append(C("quad falls back to 256x128 8 waves", 512, 768, 256, F32, QUAD, P(FAM_RING, 128, 8)))
    # ring 256 x 192 (QKV, 160 <= tiles <= CUs): 20 x 8 (map2d), 10 x 16 (xcd order; N = 3072: a strip straddles K | V at column 2048)
    for algo, tag in ((AUTO, "auto"), (SLICED, "sliced")):
        t += [C(f"qkv192 {tag} N1536 map2d q 0.5", 5120, 1536, 128, QKV, algo, P(FAM_RING, 192, 8, map2d=1), rpb=2560),
              C(f"qkv192 {tag} N3072 straddle q prod", 2560, 3072, 256, QKV, algo, P(FAM_RING, 192, 8), rpb=2560, qs="prod")]
    t += [C("qkv192 gemv items idle", 2816, 3072, 512, QKV, AUTO, P(FAM_RING, 192, 8, TAIL_GEMV, idle=True), rpb=2816, valid=2562, qs="prod"),
          C("qkv192 mfma items idle", 2816, 3072, 512, QKV, SLICED, P(FAM_RING, 192, 8, TAIL_MFMA, idle=True), rpb=2816, valid=2563),
          C("qkv192 general", 2560, 3072, 256, QKV, AUTO, P(FAM_RING, 192, 8), rpb=2560, qs="prod", regime="general")]
    # ring 256 x 128: from one tile upwards, N % 256 != 0
    pl = lambda **kw: P(FAM_RING, 128, 8, **kw)
    t += [C("ring128n one tile", 256, 128, 128, F32, SLICED, pl()), C("ring128n N384 K384 bf16+vt", 512, 384, 384, BF16, SLICED, pl(), rpb=256, vt=True),
          C("ring128n gelu+aux", 512, 384, 1024, GELU, SLICED, pl(), aux=True), C("ring128n dgelu", 512, 384, 128, DGELU, SLICED, pl()),
          C("ring128n gate out of place", 512, 384, 128, GATE, SLICED, pl(), rpb=256, inplace=False, gate_pad=8),
          C("ring128n qkv q prod", 512, 384, 256, QKV, SLICED, pl(), rpb=256, qs="prod"),
          C("ring128n valid 2 (no full tile row)", 512, 384, 512, F32, SLICED, pl(tail=TAIL_GEMV), rpb=256, valid=2),
          C("ring128n valid 20 (no full tile row)", 512, 384, 512, BF16, SLICED, pl(tail=TAIL_MFMA), rpb=256, valid=20, vt=True),
          C("ring128n valid ends on a 32-row boundary", 1024, 384, 512, F32, SLICED, pl(tail=TAIL_MFMA, idle=True), rpb=512, valid=288),
          C("ring128n valid ends on a 256-row boundary", 1024, 384, 512, F32, SLICED, pl(), rpb=512, valid=256),
          C("ring128n general", 512, 384, 384, F32, SLICED, pl(), regime="general"),
          C("ring128n general gemv items", 1024, 384, 512, BF16, SLICED, pl(tail=TAIL_GEMV, idle=True), rpb=512, valid=258, regime="general"),
          C("ring128n general mfma items", 1024, 384, 512, F32, SLICED, pl(tail=TAIL_MFMA, idle=True), rpb=512, valid=263, regime="general")]
    t += _tails("ring128n", SLICED, FAM_RING, 128, 8, (512, 2, 384), (6912, 2, 640), 384, (QKV, DGELU, GATE, F32))
    # ring 128 x 128, two K groups
    pl = lambda **kw: P(FAM_RING128, 128, 8, **kw)
    t += [C("s128 K256 f32", 256, 256, 256, F32, S128, pl()), C("s128 K768 bf16+vt", 384, 384, 768, BF16, S128, pl(), rpb=128, vt=True),
          C("s128 auto K1024 gate in place+aux", 256, 256, 1024, GATE, AUTO, pl(), rpb=128, aux=True),
          C("s128 gelu+aux+vt", 256, 256, 256, GELU, S128, pl(), rpb=256, aux=True, vt=True), C("s128 dgelu", 256, 256, 512, DGELU, S128, pl()),
          C("s128 general", 256, 384, 768, F32, S128, pl(), regime="general"),
          C("s128 general gemv items", 512, 384, 512, F32, S128, pl(tail=TAIL_GEMV, idle=True), rpb=256, valid=130, regime="general"),
          C("s128 general mfma items", 512, 384, 512, BF16, S128, pl(tail=TAIL_MFMA, idle=True), rpb=256, valid=140, regime="general")]
    t += _tails("s128", S128, FAM_RING128, 128, 8, (256, 2, 384), (1152, 2, 2048), 768, (BF16, GELU, F32, GATE))
    # 128-wide two-stage kernel
    t += [C("simple BN128 K192 f32", 2048, 4096, 192, F32, SIMPLE, P(FAM_128, 128, 4)),
          C("simple BN128 qkv valid 65", 256, 384, 128, QKV, SIMPLE, P(FAM_128, 128, 4), rpb=128, valid=65),
          C("simple BN64 N192 bf16+vt", 256, 192, 128, BF16, SIMPLE, P(FAM_128, 64, 4), rpb=128, vt=True),
          C("simple BN64 under-fill gelu+aux+vt", 256, 256, 128, GELU, SIMPLE, P(FAM_128, 64, 4), rpb=128, aux=True, vt=True),
          C("simple dgelu+vt", 256, 256, 64, DGELU, SIMPLE, P(FAM_128, 64, 4), rpb=256, vt=True),
          C("simple gate in place+aux strided gate", 256, 256, 128, GATE, SIMPLE, P(FAM_128, 64, 4), rpb=128, aux=True, gate_pad=5 * 256),
          C("simple gate out of place no bias", 256, 256, 128, GATE, SIMPLE, P(FAM_128, 64, 4), rpb=128, inplace=False, bias=False),
          C("simple batched reduction", 128, 192, 576, F32, AUTO, P(FAM_128, 64, 4), kpb=192),
          C("simple gemv_tail_rows off K576", 512, 192, 576, F32, SIMPLE, P(FAM_128, 64, 4), rpb=256, valid=130),
          C("simple gemv_tail_rows off single tile row", 256, 192, 512, F32, SIMPLE, P(FAM_128, 64, 4), rpb=128, valid=2),
          C("simple general f32", 256, 192, 576, F32, SIMPLE, P(FAM_128, 64, 4), regime="general"),
          C("simple general bf16 BN128", 256, 384, 192, QKV, SIMPLE, P(FAM_128, 128, 4), rpb=256, regime="general"),
          C("simple general gemv_tail_rows", 512, 192, 512, F32, SIMPLE, P(FAM_128, 64, 4, TAIL_GEMV, gemv_rows=1), rpb=256, valid=130, regime="general")]
    for valid in (33, 65, 97, 128):
        t.append(C(f"simple liveness valid {valid}", 256, 192, 192, BF16, SIMPLE, P(FAM_128, 64, 4), rpb=128, valid=valid, vt=True))
    for K, live, epi in ((512, 1, F32), (4096, 2, BF16), (512, 2, GELU), (1024, 1, GATE), (512, 2, DGELU)):
        t.append(C(f"simple gemv_tail_rows K{K} live {live} {EPI_NAME[epi]}", 512, 192, K, epi, SIMPLE, P(FAM_128, 64, 4, TAIL_GEMV, gemv_rows=1), rpb=256,
                   valid=128 + live, vt=epi in (BF16, GELU, DGELU), aux=epi in (GELU, GATE)))
    # split-K: 4 samples of 9 K units, cut 4 + 5; 16 tiles x 8 splits
    t += [C("split-K strided ldo", 1024, 1024, 4608, F32, AUTO, P(FAM_SPLITK, 256, 8, nsplit=8), kpb=1152, splitk=True, bias=False),
          C("split-K dense ldo", 1024, 1024, 4608, F32, SLICED, P(FAM_SPLITK, 256, 8, nsplit=8), kpb=1152, splitk=True, bias=False, dense=True)]
    names = [c["name"] for c in t]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return t


GPU_CASES = gpu_cases()


def _at(cus, cases):
    for c in cases:
        c["cus"] = cus
    return cases


def emu_cases():
    """The emulator table.  Every GPU case whose plan does not depend on the CU count and whose shape the emulator runs in seconds is taken
    over as it is (at the emulator's 6 CUs); the CU-dependent branches get DGS_EMU_CUS analogues: idle CUs / first workgroups at 6 CUs,
    map2d at 160 and 16 CUs, the 192-wide QKV tile at 8.  The true 256 x 256 kernels need 160 tiles whatever the chip: one case each on 8 and
    on 4 waves at the smallest K."""
    free = lambda c: (c["plan"]["family"] in (FAM_128, FAM_RING128) or (c["plan"]["family"] == FAM_RING and c["plan"]["bn"] == 128)) and not c["plan"]["idle"] \
        and c["plan"]["tail_form"] in (TAIL_NONE, TAIL_RING) and c["M"] * c["N"] * c["K"] <= 1 << 28
    t = [dict(c) for c in GPU_CASES if free(c)]
    t += [dict(c) for c in GPU_CASES if c["plan"]["gemv_tail_rows"] and c["K"] <= 1024]
    t += [dict(c) for c in GPU_CASES if c["name"] in ("ring128n valid 2 (no full tile row)", "ring128n valid 20 (no full tile row)")]
    # the true 256 x 256 kernels: 8 x 20 tiles, one trip of the ring; map2d needs a chip of at least 160 CUs
    t += _at(160, [C("emu ring256 map2d K128 f32", 2048, 5120, 128, F32, SLICED, P(FAM_RING, 256, 8, map2d=1)),
                   C("emu quad256 map2d K128 bf16", 2048, 5120, 128, BF16, QUAD, P(FAM_RING, 256, 4, map2d=1))])
    # map2d on the 256 x 128 tile at 16 CUs (4 x 4 tiles), and off at 6
    t += _at(16, [C("emu ring128n map2d", 1024, 512, 256, F32, SLICED, P(FAM_RING, 128, 8, map2d=1))])
    # the 192-wide QKV tile at 8 CUs: 1 x 8 tiles; N = 3072 at 16 CUs: the strip that straddles K | V
    t += _at(8, [C("emu qkv192 auto q 0.5", 256, 1536, 256, QKV, AUTO, P(FAM_RING, 192, 8), rpb=256)])
    t += _at(16, [C("emu qkv192 sliced q prod gemv items", 512, 1536, 512, QKV, SLICED, P(FAM_RING, 192, 8, TAIL_GEMV, idle=True), rpb=512, valid=258, qs="prod"),
                  C("emu qkv192 N3072 straddle", 256, 3072, 128, QKV, SLICED, P(FAM_RING, 192, 8), rpb=256, qs="prod")])
    # tails at 6 CUs: 3 full tiles leave CUs idle, 6 do not
    for tag, algo, fam, bm in (("ring128n", SLICED, FAM_RING, 256), ("s128", S128, FAM_RING128, 128)):
        for B, idle in ((1, True), (2, False)):
            rpb = 2 * bm
            w = "idle" if idle else "busy"
            t += [C(f"emu {tag} {w} gemv K512 live 1 gate", rpb * B, 384, 512, GATE, algo, P(fam, 128, 8, TAIL_GEMV, idle=idle), rpb=rpb, valid=bm + 1, aux=True),
                  C(f"emu {tag} {w} gemv K4096 live 2 bf16", rpb * B, 384, 4096, BF16, algo, P(fam, 128, 8, TAIL_GEMV, idle=idle), rpb=rpb, valid=bm + 2, vt=True),
                  C(f"emu {tag} {w} gemv K1024 live 2 gelu", rpb * B, 384, 1024, GELU, algo, P(fam, 128, 8, TAIL_GEMV, idle=idle), rpb=rpb, valid=bm + 2, vt=True, aux=True),
                  C(f"emu {tag} {w} mfma live 3 f32", rpb * B, 384, 512, F32, algo, P(fam, 128, 8, TAIL_MFMA, idle=idle), rpb=rpb, valid=bm + 3),
                  C(f"emu {tag} {w} mfma live 32 qkv", rpb * B, 384, 512, QKV, SLICED, P(FAM_RING, 128, 8, TAIL_MFMA, idle=idle), rpb=2 * 256, valid=256 + 32),
                  C(f"emu {tag} {w} mfma live 20 dgelu", rpb * B, 384, 1024, DGELU, algo, P(fam, 128, 8, TAIL_MFMA, idle=idle), rpb=rpb, valid=bm + 20, vt=True),
                  C(f"emu {tag} {w} mfma live 7 gate", rpb * B, 384, 512, GATE, algo, P(fam, 128, 8, TAIL_MFMA, idle=idle), rpb=rpb, valid=bm + 7, aux=True, inplace=False)]
    t = [c for c in t if not (c["name"].startswith("emu s128") and c["epi"] == QKV)]
    names = set()
    return [c for c in t if not (c["name"] in names or names.add(c["name"]))]


EMU_CASES = emu_cases()
# split-K on the emulator: DGS_SPLITK_MIN_ITEMS=1 lets a 256 x 256 output of 2 samples x 9 K units split (2 x 2 planes, units cut 4 + 5)
EMU_SPLITK = [C("emu split-K strided ldo", 256, 256, 2304, F32, AUTO, P(FAM_SPLITK, 256, 8, nsplit=4), kpb=1152, splitk=True, bias=False),
              C("emu split-K dense ldo", 256, 256, 2304, F32, SLICED, P(FAM_SPLITK, 256, 8, nsplit=4), kpb=1152, splitk=True, bias=False, dense=True)]
