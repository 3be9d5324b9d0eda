"""A/B of two builds of the library on the DiT GEMMs: bit-compare of the outputs -- the four GEMMs of a block at the shipped shape (one
sample at 256^2: 4,352 padded rows, 4,098 valid, incl. the two learned-token rows), then the paths that shape does not reach (the
128-wide kernel's GEMV items, the ring kernel's two-row and single-block side jobs, the LayerNorm + GEMM pair, the split-K weight
gradient) -- and alternating timed launches (HIP events) at the shipped and the training shapes.
    python tools/gemm_ab.py <base.so> [<new.so>]          (new defaults to the product library)
`base.so` is the product library of another checkout (tools/ab_build.sh swaps ONE source file, which is enough when no header changed).
Timing is ROUNDS rounds of alternating launches, base against base first: a new / base ratio means something only against the spread of
the base / base ratios of the same run.
`--cpu <rows> [<base emulator .so>]`: the bit-compare half on the CPU emulator build, small shapes (base defaults to the same library)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
import torch

from dgs_amd import _native
from dgs_amd.dit import DitOps

CPU = "--cpu" in sys.argv
if CPU:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from emu_util import emu_lib
    at = sys.argv.index("--cpu")
    DEV, M = "cpu", int(sys.argv[at + 1])
    os.environ["DGS_SPLITK_MIN_ITEMS"] = "1"                  # the split-K path at emulator-sized shapes
    L, new = M - 126, DitOps(emu_lib())
    base = DitOps(_native.open_library(os.path.abspath(sys.argv[at + 2]))) if len(sys.argv) > at + 2 else DitOps(emu_lib())
else:
    DEV, M, L = "cuda:0", 4352, 4098
    base = DitOps(_native.open_library(os.path.abspath(sys.argv[1])))
    new = DitOps(_native.open_library(os.path.abspath(sys.argv[2])) if len(sys.argv) > 2 else None)
ITERS, ROUNDS = 40, 9
g = torch.Generator(device=DEV).manual_seed(0)
bf = lambda *s: torch.randn(*s, generator=g, device=DEV).to(torch.bfloat16)
f32 = lambda *s: torch.randn(*s, generator=g, device=DEV)
W = 1024 if not CPU else 256
E = _native
failed = []


def sync():
    if not CPU:
        torch.cuda.synchronize()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def compare(name, fn):
    """fn(ops) -> tensors; every one of them, padding included (same prefill on both sides), bit for bit"""
    if not CPU:
        base.poison_lds(); new.poison_lds()
    a, b = fn(base), fn(new)
    sync()
    same = all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
    finite = all(bool(torch.isfinite(y.float()).all()) for y in b)
    if not (same and finite):
        failed.append(name)
    print(f"{name}: outputs bit-identical: {same}; finite: {finite}; max |diff| "
          f"{max(float((x.float() - y.float()).abs().max()) for x, y in zip(a, b)):.3g}", flush=True)


def time_pair(name, call_a, call_b, flops=0.0):
    """ROUNDS x ITERS alternating launches of a (base) and b; -> the per-round b / a median ratios"""
    ratios, med = [], {}
    for _ in range(3):
        call_a(); call_b()
    for _ in range(ROUNDS):
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ITERS)] for k in "ab"}
        for i in range(ITERS):
            for k, call in (("a", call_a), ("b", call_b)):
                e0, e1 = ev[k][i]
                e0.record(); call(); e1.record()
        sync()
        med = {k: sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in v)[ITERS // 2] for k, v in ev.items()}
        ratios.append(med["b"] / med["a"])
    tf = f" ({flops / med['a'] / 1e6:.0f} / {flops / med['b'] / 1e6:.0f} TFLOP/s)" if flops else ""
    print(f"    {name}: last round {med['a']:.1f} / {med['b']:.1f} us{tf}; ratios per round " + " ".join(f"{r:.3f}" for r in ratios), flush=True)
    return ratios


def verdict(name, make_call, flops=0.0):
    """base against base, then base against new: passes if the median new / base ratio lies inside the base / base spread"""
    print(f"timing {name} (median of {ITERS} alternating launches per round, preallocated outputs):", flush=True)
    bb = time_pair("base / base", make_call(base), make_call(base), flops)
    bn = time_pair("new  / base", make_call(base), make_call(new), flops)
    r = sorted(bn)[ROUNDS // 2]
    ok = min(bb) <= r <= max(bb)
    print(f"    new / base median {r:.3f}; base / base spread [{min(bb):.3f}, {max(bb):.3f}]: {'inside' if ok else 'OUTSIDE'}", flush=True)


# ---- the four GEMMs of a block at the shipped shape ----
for name, N, K, epi in [("qkv", 3 * W, W, E.EPI_QKV), ("proj", W, W, E.EPI_GATE_RESIDUAL), ("fc1", 4 * W, W, E.EPI_GELU_BF16), ("fc2", W, 4 * W, E.EPI_GATE_RESIDUAL)]:
    A, Wt, bias = bf(M, K), bf(N, K) * 0.05, f32(N)
    x0, gate = f32(M, N), f32(1, N)

    def run(ops):
        kw = dict(rows_per_batch=M, valid_rows=L)
        if epi == E.EPI_GATE_RESIDUAL:
            x = x0.clone()
            ops.gemm(A, Wt, bias, epi, out=x, gate=gate, **kw)
            return (x,)
        out = ops.gemm(A, Wt, bias, epi, **kw)
        return out if epi == E.EPI_QKV else (out,)

    compare(name, run)
    if CPU:
        continue

    def make_call(ops):
        kw = dict(rows_per_batch=M, valid_rows=L)
        if epi == E.EPI_QKV:
            qk, vt = torch.zeros(M, 2 * N // 3, dtype=torch.bfloat16, device=DEV), torch.zeros(1, N // 3, M, dtype=torch.bfloat16, device=DEV)
            return lambda: ops.gemm(A, Wt, bias, epi, out=qk, vt=vt, **kw)
        if epi == E.EPI_GELU_BF16:
            o = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
            return lambda: ops.gemm(A, Wt, bias, epi, out=o, **kw)
        x = x0.clone()
        return lambda: ops.gemm(A, Wt, bias, epi, out=x, gate=gate, **kw)

    verdict(f"{name} [{M} x {N} x {K}]", make_call, 2.0 * L * N * K)


# ---- the 128-wide kernel with its GEMV items behind the tiles (4,098 = 32 x 128 + 2 live rows), timed: proj and fc2 ----
if not CPU:
    for name, N, K in [("proj", W, W), ("fc2", W, 4 * W)]:
        A, Wt, bias, x0, gate = bf(M, K), bf(N, K) * 0.05, f32(N), f32(M, N), f32(1, N)

        def make_call(ops):
            x = x0.clone()
            return lambda: ops.gemm(A, Wt, bias, E.EPI_GATE_RESIDUAL, out=x, gate=gate, rows_per_batch=M, valid_rows=L, algo=E.GEMM_SIMPLE128)

        verdict(f"128-wide kernel + GEMV items, {name} [{M} x {N} x {K}]", make_call, 2.0 * L * N * K)


# ---- the paths the shipped shape does not reach.  One case = one (kernel, shape); every epilogue listed runs on both libraries. ----
def epilogue_runs(A, Wt, bias, x0, gate, rpb, valid, algo, epis):
    Mx, N = A.shape[0], Wt.shape[0]
    B = Mx // rpb
    kw = dict(rows_per_batch=rpb, valid_rows=valid, algo=algo)
    fill = lambda *s: torch.full(s, 7.0, dtype=torch.bfloat16, device=DEV)

    def run(ops):
        res = []
        for epi in epis:
            if epi == "f32":
                res.append(ops.gemm(A, Wt, bias, E.EPI_F32, out=torch.full((Mx, N), 7.0, device=DEV), **kw))
            elif epi == "gate":
                x, aux = x0.clone(), fill(Mx, N)
                ops.gemm(A, Wt, bias, E.EPI_GATE_RESIDUAL, out=x, gate=gate, aux=aux, **kw)
                res += [x, aux]
            elif epi == "bf16+vt":
                vt = fill(B, N, rpb)
                res += [ops.gemm(A, Wt, bias, E.EPI_BF16, out=fill(Mx, N), vt=vt, **kw), vt]
            elif epi == "gelu+aux+vt":
                aux, vt = fill(Mx, N), fill(B, N, rpb)
                res += [ops.gemm(A, Wt, bias, E.EPI_GELU_BF16, out=fill(Mx, N), aux=aux, vt=vt, **kw), aux, vt]
            elif epi == "qkv" and N % 384 == 0:
                res += list(ops.gemm(A, Wt, bias, E.EPI_QKV, out=fill(Mx, 2 * N // 3), vt=fill(B, N // 3, rpb), q_scale=0.5, **kw))
        return res
    return run


def gemm_case(name, B, rpb, valid, N, K, algo, epis):
    A, Wt, bias, x0, gate = bf(B * rpb, K), bf(N, K) * 0.05, f32(N), f32(B * rpb, N), f32(B, N)
    compare(f"{name} [{B} x {rpb} ({valid} live) x {N} x {K}] {' '.join(epis)}", epilogue_runs(A, Wt, bias, x0, gate, rpb, valid, algo, epis))


for K in (512, 4096):                                         # the 128-wide kernel's GEMV items
    gemm_case("128-wide kernel, GEMV items", 2, 256, 130, 256, K, E.GEMM_SIMPLE128, ["f32", "gate", "bf16+vt"])
# the ring kernel's two-row items: on the GPU 48 samples put N = 1536 on 288 tiles of 256 x 256 (items inside the tile workgroups) and
# N = 256 / 512 on 96 / 192 tiles of 256 x 128 (workgroups of their own); on the emulator's 6 CUs 2 samples do the same (24 / 4 / 8 tiles)
for N in (256, 512, 1536):
    for K in (1024, 2048):
        for aname, algo in (("sliced", E.GEMM_SLICED), ("quad", E.GEMM_QUAD)):
            gemm_case(f"ring kernel ({aname}), two-row items", 2 if CPU else 48, 512, 258, N, K, algo, ["f32", "gate", "gelu+aux+vt", "qkv"])
# the ring kernel's single-block MFMA items (tail_mode 1); N = 25,344 gets 256-wide tiles, so QUAD is the 4-wave kernel there
for N in (768,) if CPU else (768, 25344):
    for aname, algo in (("sliced", E.GEMM_SLICED), ("quad", E.GEMM_QUAD)):
        gemm_case(f"ring kernel ({aname}), single-block MFMA items", 2, 512, 276, N, 1024, algo, ["f32", "gelu+aux+vt", "gate", "qkv"])

for width in (512, 1024, 2048):                               # layernorm_gemm against the two-launch form, and against the base
    for N, epi in ((1536, E.EPI_QKV), (512, E.EPI_GELU_BF16)):
        x, mod, Wt, bias = f32(1024, width), f32(2, 2 * width) * 0.3, bf(N, width) * 0.05, f32(N)
        args = (x, mod[:, :width], mod[:, width:], Wt, bias, epi, 512, 258)
        name = f"layernorm_gemm width {width}, N {N}"
        compare(name, lambda ops: ops.layernorm_gemm(*args, algo=E.GEMM_SLICED, q_scale=0.7))
        h = new.layernorm(x, shift=args[1], scale=args[2], rows_per_batch=512)
        two = new.gemm(h, Wt, bias, epi, rows_per_batch=512, valid_rows=258, algo=E.GEMM_SLICED, q_scale=0.7)
        one = new.layernorm_gemm(*args, algo=E.GEMM_SLICED, q_scale=0.7)
        assert new.last_pair_shared_rows
        live = ((torch.arange(1024) % 512) < 258).to(DEV)
        same = torch.equal(bits(one[0]), bits(h)) and torch.equal(bits(one[1][live]), bits((two[0] if epi == E.EPI_QKV else two)[live]))
        if epi == E.EPI_QKV:
            same = same and torch.equal(bits(one[2]), bits(two[1]))
        if not same:
            failed.append(name + " pair")
        print(f"{name}, one launch pair against two launches (new): outputs bit-identical: {same}", flush=True)

# split-K weight gradient: dW[N, K] = sum over samples and tokens, operands [sample][feature][token]
SB, SN, SK, ST = (2, 256, 512, 1152) if CPU else (4, 1024, 1024, 4224)
dyT, xT = bf(SB, SN, ST) * 0.3, bf(SB, SK, ST) * 0.3
wgrad = lambda ops: (ops.gemm(dyT, xT, None, E.EPI_F32, out=torch.full((SN, SK), 7.0, device=DEV), shape=(SN, SK, SB * ST), k_per_batch=ST,
                              a_batch_stride=SN * ST, w_batch_stride=SK * ST, lda=ST, ldw=ST, splitk=True),)
assert new.lib.dgs_dit_gemm_splitk_bytes(SN, SK, SB * ST, ST) > 0
compare(f"split-K weight gradient [{SN} x {SK} x {SB} * {ST}]", wgrad)
if not CPU:
    def make_call(ops):                                       # (the scratch planes come from torch's caching allocator inside ops.gemm: no kernel)
        out = torch.zeros(SN, SK, device=DEV)
        return lambda: ops.gemm(dyT, xT, None, E.EPI_F32, out=out, shape=(SN, SK, SB * ST), k_per_batch=ST, a_batch_stride=SN * ST,
                                w_batch_stride=SK * ST, lda=ST, ldw=ST, splitk=True)

    verdict(f"split-K weight gradient [{SN} x {SK} x {SB} * {ST}]", make_call, 2.0 * SN * SK * SB * ST)

# ---- training forward at 4 samples: every tile also leaves a transposed copy (`vt`: [sample][feature][token], the weight-gradient
#      GEMMs' operand) -- QKV (V^T only), fc1 + GELU with aux (pre-activations) and vt, the LN-output style plain BF16 with vt ----
if not CPU:
    B4, M4 = 4, 4 * 4352
    for name, N, K, epi in [("train qkv", 3 * W, W, E.EPI_QKV), ("train fc1+gelu+vt", 4 * W, W, E.EPI_GELU_BF16), ("train bf16+vt", W, W, E.EPI_BF16)]:
        A, Wt, bias = bf(M4, K), bf(N, K) * 0.05, f32(N)

        def make_call(ops, keep=None):
            qkv = epi == E.EPI_QKV
            out = torch.zeros(M4, 2 * N // 3 if qkv else N, dtype=torch.bfloat16, device=DEV)
            vt = torch.zeros(B4, N // 3 if qkv else N, 4352, dtype=torch.bfloat16, device=DEV)
            aux = torch.zeros(M4, N, dtype=torch.bfloat16, device=DEV) if epi == E.EPI_GELU_BF16 else None
            if keep is not None:
                keep += [out, vt] + ([aux] if aux is not None else [])
            return lambda: ops.gemm(A, Wt, bias, epi, out=out, vt=vt, aux=aux, rows_per_batch=4352, valid_rows=L)

        def once(ops):
            keep = []
            make_call(ops, keep)()
            return keep

        compare(f"{name} [{M4} x {N} x {K}], outputs + transposed copies", once)
        verdict(f"{name} [{M4} x {N} x {K}]", make_call, 2.0 * B4 * L * N * K)

print("ALL BIT-IDENTICAL" if not failed else "NOT BIT-IDENTICAL: " + "; ".join(failed), flush=True)
sys.exit(1 if failed else 0)
