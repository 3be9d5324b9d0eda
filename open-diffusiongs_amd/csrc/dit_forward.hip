// dit_forward.hip -- host-side launch sequence of DGSDenoiser.image_to_gaussians (denoiser.py:306-416;
// scene variant denoiser_scene.py) on one HIP stream: no host synchronisation, no allocation, every intermediate lives
// in one caller-provided workspace (which the caller zero-fills once: padding rows are skipped by the GEMMs and must
// hold finite values).  Per DiT block: LN+modulate -> QKV GEMM (+V^T epilogue) -> flash attention ->
// proj GEMM (+gate*y+residual) -> LN+modulate -> fc1 GEMM (+GELU) -> fc2 GEMM (+gate*y+residual): 7 launches, and the
// adaLN modulation vectors of ALL blocks and both heads come from one weight-streaming GEMV up front (the
// conditioning vector is the same for every block).
#include <string.h>

#include "dit_kernels.h"
#include "raster_state.h"

namespace dgs {

struct DitWorkspace {
    float* x;        // [M, W]   residual stream, f32
    bf16_t* xn;      // [M, W]   LN+modulate output (GEMM operand)
    bf16_t* qk;      // [M, 2W]
    bf16_t* vt;      // [B, W, lpad]
    bf16_t* ao;      // [M, W]   attention output
    bf16_t* h;       // [M, 4W]  MLP hidden
    bf16_t* emb;     // [M, in_channels*ps*ps]
    float* dec;      // [M, ps*ps*C]
    float* temb;     // [B, 256]
    float* c1;       // [B, W]
    float* cvec;     // [B, W]
    float* mod;      // [B, (6*layers + 4) * W]
    float* upn;      // [B*ng, W]
    float* up;       // [B*ng, C]
    void* attn_tail; // dgs_dit_attention_tail_bytes: records + counters of the learned-token queries
    size_t attn_tail_bytes;
    static DitWorkspace carve(void* buf, const DgsDitModel* m, size_t B, size_t lpad, int L, size_t* bytes) {
        Carver c(buf);
        DitWorkspace w;
        const size_t M = B * lpad, W = (size_t)m->width;
        const size_t pp = (size_t)m->patch * m->patch;
        w.x = c.take<float>(M * W);
        w.xn = c.take<bf16_t>(M * W);
        w.qk = c.take<bf16_t>(M * 2 * W);
        w.vt = c.take<bf16_t>(M * W);
        w.ao = c.take<bf16_t>(M * W);
        w.h = c.take<bf16_t>(M * 4 * W);
        w.emb = c.take<bf16_t>(M * pp * m->in_channels);
        w.dec = c.take<float>(M * pp * m->gs_channels);
        w.temb = c.take<float>(B * 256);
        w.c1 = c.take<float>(B * W);
        w.cvec = c.take<float>(B * W);
        w.mod = c.take<float>(B * (6 * (size_t)m->layers + 4) * W);
        w.upn = c.take<float>(B * m->n_gaussians * W);
        w.up = c.take<float>(B * m->n_gaussians * m->gs_channels);
        w.attn_tail_bytes = dgs_dit_attention_tail_bytes((int)B, m->heads, L);
        w.attn_tail = c.take<char>(w.attn_tail_bytes);
        if (bytes) *bytes = c.bytes();
        return w;
    }
};

// dgs_debug_poison_lds: every 4-byte word of the workgroup's LDS = 0x7FC07FC0 (a NaN as f32 and as two bf16)
__global__ __launch_bounds__(256) void poison_lds_kernel(int words) {
    DGS_DYNAMIC_LDS(smem);
    uint32_t* w = reinterpret_cast<uint32_t*>(smem);
    for (int i = threadIdx.x; i < words; i += 256) w[i] = 0x7FC07FC0u;
    __syncthreads();
    if (w[(threadIdx.x * 97) % words] != 0x7FC07FC0u) __builtin_trap();      // keeps the stores
}

// dgs_debug_clock_probe: every workgroup runs a dependent fp32 chain until `ticks` ticks of the constant 100 MHz clock have passed;
// workgroup 0 reports how many shader-clock cycles that took.
__global__ __launch_bounds__(256) void clock_probe_kernel(long long* out, int ticks) {
    const long long w0 = wall_stamp(), c0 = cycle_stamp();
    float x = (float)threadIdx.x;
    long long w1 = w0;
    while (w1 - w0 < ticks) {
#pragma unroll
        for (int i = 0; i < 64; ++i) x = __builtin_fmaf(x, 1.0000001f, 0.5f);
        w1 = wall_stamp();
        if (w1 == w0) break;                                           // emulator: no clocks
    }
    const long long c1 = cycle_stamp();
    if (blockIdx.x == 0 && threadIdx.x == 0) { out[0] = c1 - c0; out[1] = w1 - w0; }
    if (x == 123.456f) out[2] = 1;                                     // keeps the chain
}

// ---- store policy (dit_kernels.h).  The mode is process-wide; launchers read it when they fill their parameters. ----
static int& store_policy_mode() {
    static int mode = [] {
        const char* e = getenv("DGS_STORE_POLICY");
        if (e && !strcmp(e, "plain")) return (int)DGS_STORE_PLAIN;
        if (e && !strcmp(e, "through")) return (int)DGS_STORE_THROUGH;
        if (e && *e && strcmp(e, "auto")) fprintf(stderr, "[dgs] DGS_STORE_POLICY=%s: not auto|plain|through, using auto\n", e);
        return (int)DGS_STORE_AUTO;
    }();
    return mode;
}
// auto: through exactly for the classes whose own A/B against the parent commit's library won at one-round grids
// (profiles/store_policy_ab.txt).  Multi-round grids spread their stores over the launch already and stay plain.
constexpr bool kAutoThrough[6] = {
    /* STORE_GEMM_QKV   */ false,
    /* STORE_GEMM_GELU  */ true,
    /* STORE_GEMM_GATE  */ true,
    /* STORE_GEMM_OTHER */ false,
    /* STORE_ATTENTION  */ false,
    /* STORE_LAYERNORM  */ false,
};
int store_through(StoreClass cls, bool one_round) {
    const int mode = store_policy_mode();
    if (mode != DGS_STORE_AUTO) return mode == DGS_STORE_THROUGH ? 1 : 0;
    return one_round && kAutoThrough[cls] ? 1 : 0;
}

static int token_count(const DgsDitModel* m, int V, int H, int W) { return m->n_gaussians + V * (H / m->patch) * (W / m->patch); }

}  // namespace dgs

using namespace dgs;

// 256-row granularity: the 256 x 256 GEMM tiles must not straddle samples (the 128-wide kernels skip the extra dead tile)
extern "C" int32_t dgs_dit_lpad(int32_t L) { return (L + 255) / 256 * 256; }

extern "C" size_t dgs_dit_workspace_bytes_for_tokens(const DgsDitModel* m, int32_t B, int32_t L) {
    if (!m || B <= 0 || L <= 0) return 0;
    size_t bytes = 0;
    DitWorkspace::carve(nullptr, m, (size_t)B, (size_t)dgs_dit_lpad(L), L, &bytes);
    return bytes;
}

extern "C" size_t dgs_dit_workspace_bytes(const DgsDitModel* m, int32_t B, int32_t V, int32_t H, int32_t W) {
    if (!m || B <= 0 || V <= 0 || H <= 0 || W <= 0 || m->patch <= 0) return 0;
    size_t bytes = 0;
    DitWorkspace::carve(nullptr, m, (size_t)B, (size_t)dgs_dit_lpad(token_count(m, V, H, W)), token_count(m, V, H, W), &bytes);
    return bytes;
}

#define DGS_TRY(expr) do { const int rc_ = (expr); if (rc_ != DGS_OK) { fprintf(stderr, "[dgs] %s:%d: status %d\n", __FILE__, __LINE__, rc_); return rc_; } } while (0)

namespace {
// bench.py's roofline hook: HIP events around every launch of one kernel class, on the launch stream.
struct Prof {
    void** ev; int kind, cap, n; hipStream_t st;
    bool hit(int k) const { return ev && n < cap && (k == kind || (kind == 3 && (k == 6 || k == 7))); }      // 3 = both gated-residual GEMMs (6 proj, 7 fc2)
    void before(int k) { if (hit(k)) hipEventRecord(static_cast<hipEvent_t>(ev[2 * n]), st); }
    void after(int k) { if (hit(k)) { hipEventRecord(static_cast<hipEvent_t>(ev[2 * n + 1]), st); ++n; } }
};
}  // namespace
#define DGS_PROF(k, expr) do { prof.before(k); const int rc_ = (expr); prof.after(k); if (rc_ != DGS_OK) { fprintf(stderr, "[dgs] %s:%d: status %d\n", __FILE__, __LINE__, rc_); return rc_; } } while (0)

namespace {

// DiT blocks [first, last) of the inference sequence on the residual stream ws.x (utils_transformer.py:271-290).
int run_blocks(const DgsDitModel* m, const DitWorkspace& ws, int first, int last, int B, int lpad, int L, Prof& prof, dgs_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int W = m->width, M = B * lpad, nmod = (6 * m->layers + 4) * W;
    DgsDitAttentionArgs at{};
    at.B = B; at.heads = m->heads; at.L = L; at.lpad = lpad; at.qk = ws.qk; at.vt = ws.vt; at.out = ws.ao; at.scale = 0.125f; at.q_prescaled = 1;
    at.tail_ws = ws.attn_tail; at.tail_ws_bytes = ws.attn_tail_bytes;
    const float q_scale = at.scale * 1.44269504088896341f;         // queries leave the GEMM pre-scaled for the exp2-domain softmax
    const int main_rows = L;                                       // a sample's live rows (padding rows behind them are never computed)
    static const bool rows_in_ln = !(getenv("DGS_LN_ROWS_GEMV") && atoi(getenv("DGS_LN_ROWS_GEMV")) == 0);   // 0: measurement aid (the GEMMs' own side jobs)
    for (int i = first; i < last; ++i) {
        const DgsDitLayerWeights& lw = m->layer[i];
        const float* mod = ws.mod + (size_t)i * 6 * W;   // shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
        DgsDitLayerNormArgs l1{};
        l1.rows = M; l1.width = W; l1.x = ws.x; l1.shift = mod; l1.scale = mod + W; l1.mod_stride = nmod; l1.rows_per_batch = lpad;
        l1.eps = 1e-6f; l1.out = ws.xn;
        DgsDitGemmArgs q{};
        q.M = M; q.N = 3 * W; q.K = W; q.A = ws.xn; q.lda = W; q.W = lw.qkv_w; q.ldw = W; q.bias = lw.qkv_b; q.epilogue = DGS_EPI_QKV;
        q.out = ws.qk; q.ldo = 2 * W; q.vt = ws.vt; q.rows_per_batch = lpad; q.valid_rows = main_rows;
        q.q_scale = q_scale;
        // the learned tokens' rows (L = 4096 v + 2: two rows behind a sample's last full tile) of QKV and fc1 are produced by the first
        // workgroups of the LayerNorm launch in front of the GEMM, not by side jobs inside it (layernorm_rows_gemv_kernel: same bits)
        const bool q_rows = rows_in_ln && layernorm_rows_gemv_ok(&l1, &q) && gemm_leaves_rows_out(&q);
        DGS_PROF(5, q_rows ? launch_layernorm_rows_gemv(&l1, &q, st) : launch_layernorm(&l1, st));
        DGS_PROF(2, q_rows ? launch_gemm_external_rows(&q, stream) : dgs_dit_gemm(&q, stream));
        DGS_PROF(1, dgs_dit_attention(&at, stream));
        DgsDitGemmArgs pr{};
        pr.M = M; pr.N = W; pr.K = W; pr.A = ws.ao; pr.lda = W; pr.W = lw.proj_w; pr.ldw = W; pr.bias = lw.proj_b;
        pr.epilogue = DGS_EPI_GATE_RESIDUAL; pr.out = ws.x; pr.ldo = W; pr.gate = mod + 2 * W; pr.gate_stride = nmod; pr.rows_per_batch = lpad; pr.valid_rows = main_rows;
        DGS_PROF(6, dgs_dit_gemm(&pr, stream));
        l1.shift = mod + 3 * W; l1.scale = mod + 4 * W;
        DgsDitGemmArgs f1{};
        f1.M = M; f1.N = 4 * W; f1.K = W; f1.A = ws.xn; f1.lda = W; f1.W = lw.fc1_w; f1.ldw = W; f1.bias = lw.fc1_b;
        f1.epilogue = DGS_EPI_GELU_BF16; f1.out = ws.h; f1.ldo = 4 * W; f1.rows_per_batch = lpad; f1.valid_rows = main_rows;
        const bool f_rows = rows_in_ln && layernorm_rows_gemv_ok(&l1, &f1) && gemm_leaves_rows_out(&f1);
        DGS_PROF(5, f_rows ? launch_layernorm_rows_gemv(&l1, &f1, st) : launch_layernorm(&l1, st));
        DGS_PROF(4, f_rows ? launch_gemm_external_rows(&f1, stream) : dgs_dit_gemm(&f1, stream));
        DgsDitGemmArgs f2{};
        f2.M = M; f2.N = W; f2.K = 4 * W; f2.A = ws.h; f2.lda = 4 * W; f2.W = lw.fc2_w; f2.ldw = 4 * W; f2.bias = lw.fc2_b;
        f2.epilogue = DGS_EPI_GATE_RESIDUAL; f2.out = ws.x; f2.ldo = W; f2.gate = mod + 5 * W; f2.gate_stride = nmod; f2.rows_per_batch = lpad; f2.valid_rows = main_rows;
        // (fused split-K for this 64-tile GEMM was built and measured: 66 -> 86 us, see DgsDitGemmArgs.splitk_ws / DESIGN.md section 9)
        DGS_PROF(7, dgs_dit_gemm(&f2, stream));
    }
    return DGS_OK;
}
}  // namespace

extern "C" int32_t dgs_dit_layernorm_gemm_shares_rows(const DgsDitLayerNormArgs* ln, const DgsDitGemmArgs* g) {
    return ln && g && layernorm_rows_gemv_ok(ln, g) && gemm_leaves_rows_out(g) ? 1 : 0;
}

extern "C" int dgs_dit_layernorm_gemm(const DgsDitLayerNormArgs* ln, const DgsDitGemmArgs* g, dgs_stream_t stream) {
    if (!ln || !g) return DGS_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (layernorm_rows_gemv_ok(ln, g) && gemm_leaves_rows_out(g)) {
        DGS_TRY(launch_layernorm_rows_gemv(ln, g, st));
        return launch_gemm_external_rows(g, stream);
    }
    DGS_TRY(launch_layernorm(ln, st));
    return dgs_dit_gemm(g, stream);
}

extern "C" int dgs_debug_poison_lds(dgs_stream_t stream) {
    constexpr int kBytes = 160 * 1024;
    static const bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(dgs::poison_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kBytes) == hipSuccess;
    if (!ok) return DGS_ERR_DEVICE;
    hipLaunchKernelGGL(dgs::poison_lds_kernel, dim3(2048), dim3(256), kBytes, static_cast<hipStream_t>(stream), kBytes / 4);
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}

extern "C" int dgs_debug_store_policy(int32_t policy) {
    if (policy != DGS_STORE_AUTO && policy != DGS_STORE_PLAIN && policy != DGS_STORE_THROUGH) return DGS_ERR_INVALID_ARGUMENT;
    dgs::store_policy_mode() = policy;
    return DGS_OK;
}

extern "C" int dgs_debug_clock_probe(int64_t* out, int32_t microseconds, dgs_stream_t stream) {
    if (!out || microseconds <= 0 || microseconds > 100000) return DGS_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(dgs::clock_probe_kernel, dim3(256), dim3(256), 0, static_cast<hipStream_t>(stream), reinterpret_cast<long long*>(out), microseconds * 100);
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}

extern "C" int dgs_dit_forward(const DgsDitModel* m, const DgsDitForwardArgs* a, dgs_stream_t stream) {
    if (!m || !a || a->B <= 0 || a->V <= 0 || a->H <= 0 || a->W <= 0) { fprintf(stderr, "[dgs] %s:%d: invalid argument\n", __FILE__, __LINE__); return DGS_ERR_INVALID_ARGUMENT; }
    if (m->width % 256 || m->width != m->heads * 64 || m->layers <= 0 || m->patch <= 0 || a->H % m->patch || a->W % m->patch)
        { fprintf(stderr, "[dgs] %s:%d: invalid argument\n", __FILE__, __LINE__); return DGS_ERR_INVALID_ARGUMENT; }
    // gs_channels = 11 + 3 (gaussians_sh_degree + 1)^2 (denoiser.py:96,148): degrees 0 .. 3 in the inference forward (the training calls: degree 0)
    if ((m->gs_channels != 14 && m->gs_channels != 23 && m->gs_channels != 38 && m->gs_channels != 59) || m->in_channels != 9 || (m->in_channels * m->patch * m->patch) % 64) { fprintf(stderr, "[dgs] %s:%d: invalid argument\n", __FILE__, __LINE__); return DGS_ERR_INVALID_ARGUMENT; }
    if (!a->images || !a->ray_o || !a->ray_d || !a->t || !a->workspace || !a->xyz || !a->features || !a->scaling || !a->rotation || !a->opacity)
        { fprintf(stderr, "[dgs] %s:%d: invalid argument\n", __FILE__, __LINE__); return DGS_ERR_INVALID_ARGUMENT; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int B = a->B, V = a->V, H = a->H, Wd = a->W, W = m->width, ng = m->n_gaussians, C = m->gs_channels;
    const int L = token_count(m, V, H, Wd), lpad = dgs_dit_lpad(L), M = B * lpad;
    const int pp = m->patch * m->patch, kin = m->in_channels * pp;
    size_t need = 0;
    DitWorkspace ws = DitWorkspace::carve(a->workspace, m, (size_t)B, (size_t)lpad, L, &need);
    if (a->workspace_bytes < need) return DGS_ERR_ALLOC;
    const int nmod = (6 * m->layers + 4) * W;
    Prof prof{a->prof_events, a->prof_kind, a->prof_capacity, 0, st};

    // ---- conditioning: t -> sinusoid -> MLP -> cvec; all adaLN modulations in one GEMV (denoiser.py:26-72; DiTBlock :266-272) ----
    DGS_TRY(launch_timestep(a->t, ws.temb, B, st));
    for (int b0 = 0; b0 < B; b0 += 16) {
        const int mb = B - b0 < 16 ? B - b0 : 16;
        DgsDitRowLinearArgs r{};
        r.M = mb; r.N = W; r.K = 256; r.x = ws.temb + (size_t)b0 * 256; r.W = m->t_w0; r.bias = m->t_b0; r.silu_output = 1; r.out = ws.c1 + (size_t)b0 * W;
        DGS_TRY(launch_rowlinear(&r, st));
        r.K = W; r.x = ws.c1 + (size_t)b0 * W; r.W = m->t_w1; r.bias = m->t_b1; r.silu_output = 0; r.out = ws.cvec + (size_t)b0 * W;
        DGS_TRY(launch_rowlinear(&r, st));
        r.N = nmod; r.x = ws.cvec + (size_t)b0 * W; r.silu_input = 1; r.W = m->ada_w; r.bias = m->ada_b; r.out = ws.mod + (size_t)b0 * nmod;
        DGS_TRY(launch_rowlinear(&r, st));
    }

    // ---- tokens: embed + patchify -> tokenizer GEMM -> learned tokens -> input LayerNorm (denoiser.py:312-347) ----
    // (ws.emb is NOT zeroed here: the embed kernel writes every image-token row, and the rows it never writes -- the learned tokens',
    //  whose tokenizer output must be zero, and the padding -- hold the zeros the workspace contract asks for once per shape,
    //  dgs_dit.h `workspace`; rounds 2-5 re-zeroed 5 MB per call: 5 us + a launch boundary)
    EmbedParams ep;
    ep.B = B; ep.V = V; ep.H = H; ep.W = Wd; ep.ps = m->patch; ep.lpad = lpad; ep.relative_plk = m->relative_plk;
    ep.images = a->images; ep.ray_o = a->ray_o; ep.ray_d = a->ray_d; ep.out = ws.emb;
    DGS_TRY(launch_embed(ep, st));
    DgsDitGemmArgs g{};
    g.M = M; g.N = W; g.K = kin; g.A = ws.emb; g.lda = kin; g.W = m->tok_w; g.ldw = kin; g.epilogue = DGS_EPI_F32; g.out = ws.x; g.ldo = W;
    g.rows_per_batch = lpad; g.valid_rows = L;
    DGS_TRY(dgs_dit_gemm(&g, stream));
    DGS_TRY(launch_pos_embed(m->pos_emb, ws.x, B, lpad, L, ng, W, st));
    DgsDitLayerNormArgs ln{};
    ln.rows = M; ln.width = W; ln.x = ws.x; ln.weight = m->in_ln_w; ln.eps = 1e-5f; ln.out = ws.x; ln.out_f32 = 1; ln.rows_per_batch = lpad;
    DGS_TRY(launch_layernorm(&ln, st));

    // ---- 24 x DiTBlock ----
    DGS_TRY(run_blocks(m, ws, 0, m->layers, B, lpad, L, prof, stream));
    if (a->prof_count) *a->prof_count = prof.n;
    if (a->tokens) DGS_TRY(launch_gather_tokens(ws.x, a->tokens, B, lpad, L, ng, W, st));

    // ---- heads (denoiser.py:122-136,155-164): LN(weight)+modulate -> Linear ----
    const float* mod_up = ws.mod + (size_t)m->layers * 6 * W;   // shift, scale
    const float* mod_dec = mod_up + 2 * W;
    DgsDitLayerNormArgs ld{};
    ld.rows = M; ld.width = W; ld.x = ws.x; ld.weight = m->dec_ln_w; ld.shift = mod_dec; ld.scale = mod_dec + W; ld.mod_stride = nmod;
    ld.rows_per_batch = lpad; ld.eps = 1e-5f; ld.out = ws.xn;
    DGS_TRY(launch_layernorm(&ld, st));
    DgsDitGemmArgs dg{};
    dg.M = M; dg.N = pp * C; dg.K = W; dg.A = ws.xn; dg.lda = W; dg.W = m->dec_w; dg.ldw = W; dg.epilogue = DGS_EPI_F32; dg.out = ws.dec; dg.ldo = pp * C; dg.rows_per_batch = lpad; dg.valid_rows = L;
    DGS_TRY(dgs_dit_gemm(&dg, stream));
    for (int b = 0; b < B; ++b) {
        DgsDitLayerNormArgs lu{};
        lu.rows = ng; lu.width = W; lu.x = ws.x + ((size_t)b * lpad + (L - ng)) * W; lu.weight = m->up_ln_w;
        lu.shift = mod_up + (size_t)b * nmod; lu.scale = mod_up + W + (size_t)b * nmod; lu.mod_stride = nmod; lu.rows_per_batch = ng;
        lu.eps = 1e-5f; lu.out = ws.upn + (size_t)b * ng * W; lu.out_f32 = 1;
        DGS_TRY(launch_layernorm(&lu, st));
    }
    for (int r0 = 0; r0 < B * ng; r0 += 16) {
        const int mr = B * ng - r0 < 16 ? B * ng - r0 : 16;
        DgsDitRowLinearArgs r{};
        r.M = mr; r.N = C; r.K = W; r.x = ws.upn + (size_t)r0 * W; r.W = m->up_w; r.out = ws.up + (size_t)r0 * C;
        DGS_TRY(launch_rowlinear(&r, st));
    }

    // ---- to_gs + pixel alignment (denoiser.py:103-120,370-413) ----
    GsParams gp;
    gp.B = B; gp.V = V; gp.H = H; gp.W = Wd; gp.ps = m->patch; gp.lpad = lpad; gp.ng = ng; gp.C = C; gp.scene = m->scene;
    gp.relative_plk = m->relative_plk; gp.range_near = m->range_near; gp.range_far = m->range_far;
    gp.dec = ws.dec; gp.up = ws.up; gp.ray_o = a->ray_o; gp.ray_d = a->ray_d;
    gp.xyz = a->xyz; gp.features = a->features; gp.scaling = a->scaling; gp.rotation = a->rotation; gp.opacity = a->opacity;
    gp.aligned = a->aligned_xyz;
    DGS_TRY(launch_gaussians(gp, st));
    return DGS_OK;
}

// DGSDenoiser.run_layers(first, last) (denoiser.py:441-447): blocks [first, last) applied to a token tensor in the reference's
// order ([gaussian tokens, image tokens]) under the conditioning vector c = t_embedder(t).  What torch.utils.checkpoint wraps
// in the reference; here an inference-mode utility (the training path recomputes inside dgs_dit_backward).
extern "C" int dgs_dit_run_blocks(const DgsDitModel* m, const DgsDitRunBlocksArgs* a, dgs_stream_t stream) {
    if (!m || !a || a->B <= 0 || a->B > 16 || a->L <= m->n_gaussians || a->first < 0 || a->last > m->layers || a->first > a->last ||
        !a->tokens_in || !a->tokens_out || !a->cvec || !a->workspace)
        return DGS_ERR_INVALID_ARGUMENT;
    if (a->V > 0 && (a->L - m->n_gaussians) % a->V) return DGS_ERR_INVALID_ARGUMENT;     // V is a consistency check only (0: not given)
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int B = a->B, W = m->width, ng = m->n_gaussians, L = a->L, lpad = dgs_dit_lpad(L);
    const int nmod = (6 * m->layers + 4) * W;
    size_t need = 0;
    DitWorkspace ws = DitWorkspace::carve(a->workspace, m, (size_t)B, (size_t)lpad, L, &need);
    if (a->workspace_bytes < need) return DGS_ERR_ALLOC;
    DgsDitRowLinearArgs r{};
    r.M = B; r.N = nmod; r.K = W; r.x = a->cvec; r.silu_input = 1; r.W = m->ada_w; r.bias = m->ada_b; r.out = ws.mod;
    DGS_TRY(launch_rowlinear(&r, st));
    DGS_TRY(launch_scatter_tokens(a->tokens_in, ws.x, B, lpad, L, ng, W, st));
    Prof prof{nullptr, 0, 0, 0, st};
    DGS_TRY(run_blocks(m, ws, a->first, a->last, B, lpad, L, prof, stream));
    DGS_TRY(launch_gather_tokens(ws.x, a->tokens_out, B, lpad, L, ng, W, st));
    return DGS_OK;
}
