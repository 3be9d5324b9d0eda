"""Store policy of the forward kernels' bulk outputs (dgs_debug_store_policy: plain write-back stores or sc1 write-through stores):
what test_store_policy_emu.py and test_store_policy_gpu.py share.  The policy changes how a value leaves the CU, never the value or
its address: every case runs under PLAIN and under THROUGH on the same inputs, and every byte of every output buffer -- written rows,
unwritten rows, slack columns -- must be the same under both.  The guard bands around the buffers are checked after every launch."""
import contextlib
import os

import gemm_util as G
from dgs_amd import _native
from rowkernel_util import bit_equal

AUTO, PLAIN, THROUGH = _native.STORE_AUTO, _native.STORE_PLAIN, _native.STORE_THROUGH
POLICY_NAME = {PLAIN: "plain", THROUGH: "through"}


@contextlib.contextmanager
def policy_setter(lib):
    """-> set(policy); on exit the process is back on the policy it started with (DGS_STORE_POLICY, default auto)."""
    start = {"plain": PLAIN, "through": THROUGH}.get(os.environ.get("DGS_STORE_POLICY", "auto"), AUTO)

    def set_policy(p):
        rc = lib.dgs_debug_store_policy(p)
        assert rc == 0, ("dgs_debug_store_policy", p, rc)

    try:
        yield set_policy
    finally:
        lib.dgs_debug_store_policy(start)


# the (plan family) x (epilogue) pairs whose row-major pass takes the policy
FAMILIES = (("128-wide", lambda p: p["family"] == G.FAM_128),
            ("ring 256x256", lambda p: p["family"] == G.FAM_RING and p["bn"] == 256 and p["waves"] == 8),
            ("ring 256x192", lambda p: p["family"] == G.FAM_RING and p["bn"] == 192),
            ("ring 256x128", lambda p: p["family"] == G.FAM_RING and p["bn"] == 128),
            ("ring 128x128", lambda p: p["family"] == G.FAM_RING128))
EPILOGUES = (("f32", lambda c: c["epi"] == G.F32), ("bf16", lambda c: c["epi"] == G.BF16), ("gelu", lambda c: c["epi"] == G.GELU),
             ("gate in place", lambda c: c["epi"] == G.GATE and c["inplace"]), ("gate with resid", lambda c: c["epi"] == G.GATE and not c["inplace"]),
             ("qkv", lambda c: c["epi"] == G.QKV))


def _size(c):
    return c["M"] * c["N"] * c["K"]


def gemm_subset(table, families):
    """Of a gemm_util case table: per (family, epilogue) pair the exact-regime case with the smallest M N K among those whose every tile
    row is a full one (among all, where the table has the pair only with side items), + the strip that straddles K | V on the 192-wide tile, + the smallest case with valid_rows < rows_per_batch, + the
    smallest with two-row GEMV items."""
    plain_rows = [c for c in table if c["regime"] == "exact" and not c["splitk"] and not c["kpb"] and c["plan"]["tail_form"] == G.TAIL_NONE]
    picked = []
    for fname, fam in FAMILIES:
        if fname not in families:
            continue
        for _, epi in EPILOGUES:
            hits = [c for c in plain_rows if fam(c["plan"]) and epi(c) and not 0 < c["valid"] < (c["rpb"] or c["M"])]
            if not hits:                                     # the pair only exists with side items (the 128 x 128 ring's out-of-place gate)
                hits = [c for c in table if c["regime"] == "exact" and not c["splitk"] and fam(c["plan"]) and epi(c)]
            if hits:
                picked.append(min(hits, key=_size))
    picked += [min((c for c in table if "straddle" in c["name"]), key=_size, default=None)]
    picked += [min((c for c in plain_rows if 0 < c["valid"] < (c["rpb"] or c["M"])), key=_size, default=None)]
    picked += [min((c for c in table if c["regime"] == "exact" and c["plan"]["tail_form"] == G.TAIL_GEMV), key=_size, default=None)]
    names, out = set(), []
    for c in picked:
        if c is not None and c["name"] not in names:
            names.add(c["name"])
            out.append(c)
    return out


def run_gemm_both(lib, device, c, set_policy, monkeypatch, before=None):
    """gemm_util.run_case (plan assertion, guard bands, the exactness rules against fp64) under both policies; the plan must report
    the policy that ran, and every output buffer must be the same bit for bit."""
    seen = {}
    for pol in (PLAIN, THROUGH):
        set_policy(pol)
        kept = {}

        def spy(run, kept=kept):
            r = G.R.twice(run)
            kept.update(r)
            return r

        monkeypatch.setattr(G, "twice", spy)
        plan = G.run_case(lib, device, c, before=before)
        assert plan["store_policy"] == pol, (c["name"], "the plan reports store policy", plan["store_policy"], "under", POLICY_NAME[pol])
        assert kept, (c["name"], "no output captured")
        seen[pol] = kept
    assert seen[PLAIN].keys() == seen[THROUGH].keys()
    for k in seen[PLAIN]:
        assert bit_equal(seen[PLAIN][k], seen[THROUGH][k]), (c["name"], k, "differs between the plain and the through store policy")


def run_pair_both(lib, device, set_policy, width, epi, before=None, B=2, rpb=512, valid=258):
    """dgs_dit_layernorm_gemm in the form that shares rows (gemm_util.check_layernorm_gemm's shape: the learned tokens' output rows come
    from the first workgroups of the LayerNorm launch, layernorm_rows_gemv_kernel) under both policies, into ONE set of guarded buffers
    that is refilled with the sentinel in front of each run: the LayerNorm output, the GEMM output and V^T must be the same bit for bit,
    and the rows the plan does not write must still hold the sentinel.  Width 1024 and up is where the through form of the LayerNorm rows
    stores two lane-pair pieces per row in a row (the shape at which a 16-byte store's data registers were once overwritten too early)."""
    import ctypes

    import torch

    import rowkernel_util as R
    dev = torch.device(device)
    qkv = epi == G.QKV
    N, M = (1536 if qkv else 512), B * rpb
    c = G.C(f"pair width {width} {G.EPI_NAME[epi]}", M, N, width, epi, G.SLICED, G.P(G.FAM_RING, 128, 8, G.TAIL_GEMV, idle=True), rpb=rpb, valid=valid, dense=True)
    g = torch.Generator().manual_seed(width + N)
    x = torch.randn(M, width, generator=g).to(dev)
    mod = (torch.randn(B, 2 * width, generator=g) * 0.3).to(dev)
    W = (torch.randn(N, width, generator=g) * 0.05).bfloat16().to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    ar = R.Arena(dev)
    bufs = {"xn": ar.take((M, width), torch.bfloat16, G.SENTINEL), "out": ar.take((M, 2 * N // 3 if qkv else N), torch.bfloat16, G.SENTINEL)}
    if qkv:
        bufs["vt"] = ar.take((B, N // 3, rpb), torch.bfloat16, G.SENTINEL)
    ln = _native.DgsDitLayerNormArgs()
    ln.rows, ln.width, ln.x, ln.shift, ln.scale, ln.mod_stride = M, width, x.data_ptr(), mod.data_ptr(), mod.data_ptr() + 4 * width, 2 * width
    ln.rows_per_batch, ln.eps, ln.out = rpb, 1e-6, bufs["xn"].data_ptr()
    a = _native.DgsDitGemmArgs()
    a.M, a.N, a.K, a.A, a.lda, a.W, a.ldw = M, N, width, bufs["xn"].data_ptr(), width, W.data_ptr(), width
    a.bias, a.epilogue, a.out, a.ldo = bias.data_ptr(), epi, bufs["out"].data_ptr(), bufs["out"].shape[1]
    a.vt = bufs["vt"].data_ptr() if qkv else None
    a.rows_per_batch, a.valid_rows, a.algo, a.q_scale = rpb, valid, G.SLICED, 0.5
    assert lib.dgs_dit_layernorm_gemm_shares_rows(ctypes.byref(ln), ctypes.byref(a)) == 1, (c["name"], "the pair does not take the shared-rows form")
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
    seen = {}
    for pol in (PLAIN, THROUGH):
        set_policy(pol)
        for t in bufs.values():
            t.fill_(G.SENTINEL)
        plan = G.plan_of(lib, c)
        assert plan["store_policy"] == pol and plan["tail_form"] == G.TAIL_GEMV, (c["name"], plan)
        if before:
            before()
        rc = lib.dgs_dit_layernorm_gemm(ctypes.byref(ln), ctypes.byref(a), stream)
        assert rc == 0, (c["name"], "dgs_dit_layernorm_gemm", rc)
        ar.check()
        written = G.written_rows(c, plan).to(dev)
        assert bool(torch.isfinite(bufs["xn"].float()).all()) and bool(torch.isfinite(bufs["out"].float()[written]).all())
        assert R.all_equal(bufs["out"].float()[~written], G.SENTINEL), (c["name"], POLICY_NAME[pol], "rows the plan does not write were written")
        if qkv:
            assert R.all_equal(bufs["vt"].float().transpose(1, 2).reshape(M, N // 3)[~written], G.SENTINEL), (c["name"], POLICY_NAME[pol], "V^T columns of unwritten rows")
        seen[pol] = {k: v.clone() for k, v in bufs.items()}
    for k in seen[PLAIN]:
        assert bit_equal(seen[PLAIN][k], seen[THROUGH][k]), (c["name"], k, "differs between the plain and the through store policy")
    # an independent reference for the LayerNorm rows (fp64; bf16 output: half an ulp of values up to ~8 + the fp32 arithmetic)
    ref = torch.nn.functional.layer_norm(x.double(), (width,), eps=1e-6) * (1 + mod[:, width:].double().repeat_interleave(rpb, 0)) + mod[:, :width].double().repeat_interleave(rpb, 0)
    assert float((seen[THROUGH]["xn"].double() - ref).abs().max()) < 0.05
