// lpips.hip -- LPIPS-VGG forward and input gradient (include/dgs_lpips.h states the network, the layouts and the arithmetic): a 3x3
// convolution as an implicit GEMM on the f32-input MFMA, the 2x2 maximum pool, the tap kernel, their backward forms and the two
// whole sequences.
//
// conv3x3_kernel<WM, WN, VEC, GRAD>.  C[m][co] = sum_k A[m][k] B[k][co], m = flat pixel (n, h, w) of the channels-last activation,
// k = (3 ky + kx) Cin + ci, A[m][k] = x[n][h + ky - 1][w + kx - 1][ci] or 0 outside the image, B = the packed weights.  No im2col
// matrix exists in memory: a workgroup of 256 threads (4 waves) owns BM = 64 WM consecutive pixels and BN = 64 WN output channels and
// walks K in chunks of 32.  Per chunk it stages A^T (32 x BM, pitch BM + 1) and B (32 x BN) in LDS; a wave owns 64 x 64 of the tile
// as 2 x 2 v_mfma_f32_32x32x2_f32 accumulators (4 independent chains, 64 accumulator registers) and feeds each MFMA step with four
// ds_read_b32 whose lanes read consecutive floats (conflict-free).  Tiles are flat in m, so a tile may cross rows and images; every
// staged element tests its own (h, w); a 32-row strip of a wave that holds no pixel at all takes no MFMA, and nothing is stored past M.
//   VEC (Cin % 32 == 0, 16-byte aligned x): a chunk lies inside one filter tap; a thread fetches 16 bytes of one pixel's channels
//       (8 threads cover the 128 contiguous bytes of a pixel), next chunk's fetches are issued before this chunk's MFMAs, and the four
//       floats go to four rows of A^T (pitch BM + 1: a 32-lane group writes 32 different banks).
//   scalar (any Cin; the first layer, K = 27 padded to 32 with zeros, which is exact): one float per thread and element.
// The epilogue adds the bias, applies the ReLU and stores 128 contiguous bytes per 32 lanes.
// Each output element is one accumulator register and so one fma chain over k in increasing order, wherever its tile lies.
//
// Not done here: no LDS halo patch shared by the nine taps (the nine shifted reads of a pixel are L1 / L2 hits), no double-buffered LDS.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), no scratch anywhere:
//   conv3x3_kernel<2, 2, vec / scalar>   86 / 100 VGPRs + 64 AGPRs, 32,896 B LDS, 3 waves per SIMD
//   conv3x3_kernel<4, 1, vec / scalar>   107 / 121 VGPRs + 64 AGPRs, 41,088 B LDS, 2 waves per SIMD
// GRAD: the convolution's data gradient is this kernel on the flipped, transposed operand (lpips_pack_transposed_kernel writes it from
// the torch tensor), the same chain over k = (3 ky' + kx') Cout + co, with the compile-time epilogue (mask > 0 ? acc : 0) + add in place
// of bias and ReLU; the forward's instantiations are what they were (the resources above are unchanged).  Same remarks, no scratch:
//   conv3x3_kernel<2, 2, vec / scalar, GRAD>   83 / 100 VGPRs + 64 AGPRs, 32,896 B LDS, 3 waves per SIMD
//   conv3x3_kernel<4, 1, vec / scalar, GRAD>   107 / 121 VGPRs + 64 AGPRs, 41,088 B LDS, 2 waves per SIMD
// The first layer's gradient (64 -> 3) takes the <4, 1> tile with its 3 output channels padded to 64: about twenty times the work its
// shape needs, the cost of one 64 -> 64 layer; there is no dedicated kernel for it.
// Measured (MI355X, rocprofv3 kernel trace, profiles/lpips_kernel_stats.txt): the thirteen convolutions of 32 images of 256^2 take
// 13.9 ms, 59 % of the 157 TF fp32-matrix peak from shape FLOPs; pools, taps and the input kernel together 0.9 ms.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "dgs_lpips.h"
#include "lpips_mfma.h"

namespace dgs {

constexpr int LP_KC = 32;                 // K chunk
constexpr int LP_PIXEL_BUDGET = 1 << 20;  // images * H * W pushed through the network at once
typedef float lpips_f32x4 __attribute__((ext_vector_type(4)));   // 16-byte fetches (HIP's float4 struct kept the staging registers in scratch)

template <int WM, int WN, bool VEC, bool GRAD>
__global__ __launch_bounds__(256) void conv3x3_kernel(DgsConv3x3Args a, int Cp, int Kp, const float* mask, const float* add) {
    constexpr int BM = 64 * WM, BN = 64 * WN, AS = BM + 1;
    constexpr int AV = BM / 32;           // 16-byte fetches of A per thread and chunk (VEC)
    constexpr int BV = BN / 32;           // 16-byte fetches of B per thread and chunk
    __shared__ float As[LP_KC * AS];
    __shared__ __attribute__((aligned(16))) float Bs[LP_KC * BN];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int HW = a.H * a.W;
    const long long M = (long long)a.N * HW;
    const long long m0 = (long long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int nchunks = Kp / LP_KC;

    // VEC: this thread's pixel slots p = (t >> 3) + 32 i, channel quad c4 = t & 7
    int ph[AV], pw[AV];
    if (VEC) {
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            const long long m = m0 + (t >> 3) + 32 * i;
            if (m < M) {
                const int r = (int)(m % HW);
                ph[i] = r / a.W;
                pw[i] = r - ph[i] * a.W;
            } else {
                ph[i] = -4;               // fails every row test
                pw[i] = 0;
            }
        }
    }

    lpips_f32x4 av[AV], bv[BV];
    auto fetch = [&](int c) {
#pragma unroll
        for (int j = 0; j < BV; ++j) {
            const int idx = t + 256 * j, k = idx / (BN / 4), q = idx % (BN / 4);
            bv[j] = *reinterpret_cast<const lpips_f32x4*>(a.weights + (size_t)(c * LP_KC + k) * Cp + n0 + 4 * q);
        }
        if (VEC) {
            const int tap = (c * LP_KC) / a.Cin, ci0 = c * LP_KC - tap * a.Cin;
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
#pragma unroll
            for (int i = 0; i < AV; ++i) {
                const int hh = ph[i] + dy, ww = pw[i] + dx;
                av[i] = lpips_f32x4{0.f, 0.f, 0.f, 0.f};
                if (hh >= 0 && hh < a.H && ww >= 0 && ww < a.W) {
                    const long long m = m0 + (t >> 3) + 32 * i + dy * a.W + dx;
                    av[i] = *reinterpret_cast<const lpips_f32x4*>(a.x + (size_t)m * a.Cin + ci0 + 4 * (t & 7));
                }
            }
        }
    };
    auto stage = [&](int c) {
#pragma unroll
        for (int j = 0; j < BV; ++j) *reinterpret_cast<lpips_f32x4*>(Bs + 4 * (t + 256 * j)) = bv[j];
        if (VEC) {
#pragma unroll
            for (int i = 0; i < AV; ++i) {
                float* d = As + (4 * (t & 7)) * AS + (t >> 3) + 32 * i;
                d[0] = av[i].x; d[AS] = av[i].y; d[2 * AS] = av[i].z; d[3 * AS] = av[i].w;
            }
        } else {
            const int kl = t & 31, k = c * LP_KC + kl;
            const int tap = k / a.Cin, ci = k - tap * a.Cin;
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
            for (int i = 0; i < BM / 8; ++i) {
                const int p = (t >> 5) + 8 * i;
                const long long m = m0 + p;
                float v = 0.f;
                if (m < M && tap < 9) {
                    const int r = (int)(m % HW), h = r / a.W, w = r - h * a.W;
                    const int hh = h + dy, ww = w + dx;
                    if (hh >= 0 && hh < a.H && ww >= 0 && ww < a.W) v = a.x[(size_t)(m + dy * a.W + dx) * a.Cin + ci];
                }
                As[kl * AS + p] = v;
            }
        }
    };

    lpips_f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    // wave-uniform: which of this wave's two 32-row strips hold a pixel at all (a strip without one takes no MFMA; it stores nothing)
    const bool live0 = m0 + wm * 64 < M, live1 = m0 + wm * 64 + 32 < M;
    fetch(0);
    for (int c = 0; c < nchunks; ++c) {
        __syncthreads();                  // the previous chunk's reads of As / Bs are done
        stage(c);
        __syncthreads();
        if (c + 1 < nchunks) fetch(c + 1);
        const float* ar = As + (lane >> 5) * AS + wm * 64 + (lane & 31);
        const float* br = Bs + (lane >> 5) * BN + wn * 64 + (lane & 31);
        if (live1) {
#pragma unroll 4
            for (int kk = 0; kk < LP_KC / 2; ++kk) {
                const float a0 = ar[2 * kk * AS], a1 = ar[2 * kk * AS + 32];
                const float b0 = br[2 * kk * BN], b1 = br[2 * kk * BN + 32];
                acc[0] = mfma_f32_32x32x2(a0, b0, acc[0]);
                acc[1] = mfma_f32_32x32x2(a0, b1, acc[1]);
                acc[2] = mfma_f32_32x32x2(a1, b0, acc[2]);
                acc[3] = mfma_f32_32x32x2(a1, b1, acc[3]);
            }
        } else if (live0) {               // the last tile of the image batch: its upper 32 rows hold no pixel
#pragma unroll 4
            for (int kk = 0; kk < LP_KC / 2; ++kk) {
                const float a0 = ar[2 * kk * AS];
                const float b0 = br[2 * kk * BN], b1 = br[2 * kk * BN + 32];
                acc[0] = mfma_f32_32x32x2(a0, b0, acc[0]);
                acc[1] = mfma_f32_32x32x2(a0, b1, acc[1]);
            }
        }
    }

#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int co = n0 + wn * 64 + nt * 32 + (lane & 31);
            if (co >= a.Cout) continue;
            if constexpr (GRAD) {         // the data gradient's epilogue: (mask > 0 ? acc : 0) + add; add may be y itself
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long long m = m0 + wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (m >= M) continue;
                    const size_t o = (size_t)m * a.Cout + co;
                    float v = acc[mt * 2 + nt][r];
                    if (mask && !(mask[o] > 0.f)) v = 0.f;
                    if (add) v += add[o];
                    a.y[o] = v;
                }
            } else {
                const float b = a.bias ? a.bias[co] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long long m = m0 + wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (m >= M) continue;
                    float v = acc[mt * 2 + nt][r] + b;
                    if (a.relu) v = fmaxf(v, 0.f);
                    a.y[(size_t)m * a.Cout + co] = v;
                }
            }
        }
}

__global__ __launch_bounds__(256) void lpips_pack_kernel(DgsLpipsPackArgs a, int Cp, int Kp) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)Kp * Cp) return;
    const int k = (int)(i / Cp), co = (int)(i % Cp);
    const int tap = k / a.Cin, ci = k - tap * a.Cin;
    a.packed[i] = (tap < 9 && co < a.Cout) ? a.w[((size_t)co * a.Cin + ci) * 9 + tap] : 0.f;
}

// the operand of the data gradient: the convolution Cout -> Cin on w'[ci][co][ky][kx] = w[co][ci][2 - ky][2 - kx], so
// packed[k = tap' Cout + co][ci] = w[co][ci][8 - tap']; Kp, Cp are those of that convolution (9 Cout and Cin rounded up)
__global__ __launch_bounds__(256) void lpips_pack_transposed_kernel(DgsLpipsPackArgs a, int Cp, int Kp) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)Kp * Cp) return;
    const int k = (int)(i / Cp), ci = (int)(i % Cp);
    const int tap = k / a.Cout, co = k - tap * a.Cout;
    a.packed[i] = (tap < 9 && ci < a.Cin) ? a.w[((size_t)co * a.Cin + ci) * 9 + (8 - tap)] : 0.f;
}

__global__ __launch_bounds__(256) void maxpool2x2_kernel(DgsMaxPool2x2Args a, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int Ho = a.H / 2, Wo = a.W / 2;
    const int c = (int)(i % a.C);
    long long r = i / a.C;
    const int wo = (int)(r % Wo);
    r /= Wo;
    const int ho = (int)(r % Ho);
    const long long n = r / Ho;
    const float* p = a.x + (((size_t)n * a.H + 2 * ho) * a.W + 2 * wo) * a.C + c;
    const size_t row = (size_t)a.W * a.C;
    a.y[i] = fmaxf(fmaxf(p[0], p[a.C]), fmaxf(p[row], p[row + a.C]));
}

// one thread per element of dx: it receives its window's dy if it is the first maximum of the window in (row, column) order
__global__ __launch_bounds__(256) void maxpool2x2_backward_kernel(DgsMaxPool2x2BackwardArgs a, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int Ho = a.H / 2, Wo = a.W / 2;
    const int c = (int)(i % a.C);
    long long r = i / a.C;
    const int w = (int)(r % a.W);
    r /= a.W;
    const int h = (int)(r % a.H);
    const long long n = r / a.H;
    float v = 0.f;
    if (h < 2 * Ho && w < 2 * Wo) {
        const int ho = h >> 1, wo = w >> 1;
        const float* p = a.x + (((size_t)n * a.H + 2 * ho) * a.W + 2 * wo) * a.C + c;
        const size_t row = (size_t)a.W * a.C;
        float best = p[0];
        int at = 0;
        if (p[a.C] > best) { best = p[a.C]; at = 1; }
        if (p[row] > best) { best = p[row]; at = 2; }
        if (p[row + a.C] > best) at = 3;
        if (at == 2 * (h & 1) + (w & 1)) v = a.dy[(((size_t)n * Ho + ho) * Wo + wo) * a.C + c];
    }
    if (a.relu_mask && !(a.x[i] > 0.f)) v = 0.f;
    if (a.add) v += a.add[i];
    a.dx[i] = v;
}

// ds [images, HW, 3] channels-last -> torch's layout, divided by the scale: image img goes to grad0[first + img] (img < cn) or
// grad1[first + img - cn]
__global__ __launch_bounds__(256) void lpips_input_backward_kernel(const float* ds, const float* scale, int first, int cn, int images, int HW,
                                                                   float* grad0, float* grad1) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)images * HW) return;
    const int img = (int)(i / HW), p = (int)(i % HW);
    float* dst = (img < cn ? grad0 + (size_t)(first + img) * 3 * HW : grad1 + (size_t)(first + img - cn) * 3 * HW) + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[(size_t)c * HW] = ds[i * 3 + c] / scale[c];
}

// images [0, cn) of the batch come from x0[first ...], images [cn, 2 cn) from x1[first ...]; out is channels-last and scaled
__global__ __launch_bounds__(256) void lpips_input_kernel(const float* x0, const float* x1, const float* shift, const float* scale, int first,
                                                          int cn, int HW, float* out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2LL * cn * HW) return;
    const int img = (int)(i / HW), p = (int)(i % HW);
    const float* src = (img < cn ? x0 + (size_t)(first + img) * 3 * HW : x1 + (size_t)(first + img - cn) * 3 * HW) + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[i * 3 + c] = (src[(size_t)c * HW] - shift[c]) / scale[c];
}

__device__ __forceinline__ float lpips_wave_sum(float v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);      // a + b == b + a: every lane ends with the same bits
    return v;
}

// one wave per pixel: workspace[pixel] = sum_c lin[c] (f0 / (|f0| + eps) - f1 / (|f1| + eps))^2
__global__ __launch_bounds__(256) void lpips_tap_pixel_kernel(DgsLpipsTapArgs a, long long pixels) {
    const int lane = threadIdx.x & 63;
    const long long pix = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= pixels) return;
    const float* f0 = a.f0 + (size_t)pix * a.C;
    const float* f1 = a.f1 + (size_t)pix * a.C;
    float s0 = 0.f, s1 = 0.f;
    for (int c = lane; c < a.C; c += 64) {
        s0 += f0[c] * f0[c];
        s1 += f1[c] * f1[c];
    }
    const float n0 = sqrtf(lpips_wave_sum(s0)) + 1e-10f, n1 = sqrtf(lpips_wave_sum(s1)) + 1e-10f;
    float d = 0.f;
    for (int c = lane; c < a.C; c += 64) {
        const float e = f0[c] / n0 - f1[c] / n1;
        d += a.lin[c] * (e * e);
    }
    d = lpips_wave_sum(d);
    if (lane == 0) a.workspace[pix] = d;
}

// one wave per pixel, the channel sums in the forward's lane order and butterfly (include/dgs_lpips.h 'The input gradient', tap).
// An element whose own f is 0 is written as 0 without evaluating its formula, so a pixel whose vector is all zero (r = 0) gives zeros.
__global__ __launch_bounds__(256) void lpips_tap_backward_kernel(DgsLpipsTapBackwardArgs a, long long pixels) {
    const int lane = threadIdx.x & 63;
    const long long pix = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= pixels) return;
    const float* f0 = a.f0 + (size_t)pix * a.C;
    const float* f1 = a.f1 + (size_t)pix * a.C;
    float s0 = 0.f, s1 = 0.f;
    for (int c = lane; c < a.C; c += 64) {
        s0 += f0[c] * f0[c];
        s1 += f1[c] * f1[c];
    }
    const float r0 = sqrtf(lpips_wave_sum(s0)), r1 = sqrtf(lpips_wave_sum(s1));
    const float n0 = r0 + 1e-10f, n1 = r1 + 1e-10f;
    float A0 = 0.f, A1 = 0.f;
    for (int c = lane; c < a.C; c += 64) {
        const float le = a.lin[c] * (f0[c] / n0 - f1[c] / n1);
        A0 += le * f0[c];
        A1 += le * f1[c];
    }
    A0 = lpips_wave_sum(A0);
    A1 = lpips_wave_sum(A1);
    const float k = 2.f / (float)(a.H * a.W);
    float* g0 = a.g0 + (size_t)pix * a.C;
    float* g1 = a.g1 ? a.g1 + (size_t)pix * a.C : nullptr;
    for (int c = lane; c < a.C; c += 64) {
        const float le = a.lin[c] * (f0[c] / n0 - f1[c] / n1);
        g0[c] = f0[c] == 0.f ? 0.f : k * (le / n0 - f0[c] * A0 / (n0 * n0 * r0));
        if (g1) g1[c] = f1[c] == 0.f ? 0.f : k * (f1[c] * A1 / (n1 * n1 * r1) - le / n1);
    }
}

__global__ __launch_bounds__(256) void lpips_tap_mean_kernel(DgsLpipsTapArgs a) {
    __shared__ float red[256];
    const int n = blockIdx.x, HW = a.H * a.W;
    const float* v = a.workspace + (size_t)n * HW;
    float s = 0.f;
    for (int p = threadIdx.x; p < HW; p += 256) s += v[p];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.out[(size_t)n * a.out_stride] = red[0] / (float)HW;
}

__global__ __launch_bounds__(256) void lpips_finish_kernel(const float* taps, int cn, float* out, float* per_tap) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= cn) return;
    const float* d = taps + n * DGS_LPIPS_TAPS;
    out[n] = (((d[0] + d[1]) + d[2]) + d[3]) + d[4];
    if (per_tap)
        for (int k = 0; k < DGS_LPIPS_TAPS; ++k) per_tap[n * DGS_LPIPS_TAPS + k] = d[k];
}

static inline int lp_round_up(int v, int m) { return (v + m - 1) / m * m; }
static inline bool lp_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline unsigned lp_blocks(long long n) { return (unsigned)((n + 255) / 256); }

static bool conv_ok(const DgsConv3x3Args* a) {
    return a && a->N >= 1 && a->H >= 1 && a->W >= 1 && a->Cin >= 1 && a->Cout >= 1 && a->x && a->weights && a->y && lp_aligned16(a->weights) &&
           (long long)a->N * a->H * a->W < 2147483647LL - 256 && (long long)a->N * a->H * a->W * (a->Cin > a->Cout ? a->Cin : a->Cout) < (1LL << 40) &&
           (long long)a->Cin * 9 < (1 << 24) && a->Cout < (1 << 24);
}

static void conv_launch(const DgsConv3x3Args& a, hipStream_t st) {
    const int Kp = lp_round_up(9 * a.Cin, LP_KC), Cp = lp_round_up(a.Cout, 64);
    const long long M = (long long)a.N * a.H * a.W;
    const bool vec = a.Cin % LP_KC == 0 && lp_aligned16(a.x);
    const float* none = nullptr;
    if (Cp % 128 == 0) {
        const dim3 grid((unsigned)((M + 127) / 128), Cp / 128);
        if (vec) hipLaunchKernelGGL((conv3x3_kernel<2, 2, true, false>), grid, dim3(256), 0, st, a, Cp, Kp, none, none);
        else hipLaunchKernelGGL((conv3x3_kernel<2, 2, false, false>), grid, dim3(256), 0, st, a, Cp, Kp, none, none);
    } else {
        const dim3 grid((unsigned)((M + 255) / 256), Cp / 64);
        if (vec) hipLaunchKernelGGL((conv3x3_kernel<4, 1, true, false>), grid, dim3(256), 0, st, a, Cp, Kp, none, none);
        else hipLaunchKernelGGL((conv3x3_kernel<4, 1, false, false>), grid, dim3(256), 0, st, a, Cp, Kp, none, none);
    }
}

// the data gradient: the convolution Cout -> Cin of dy on the transposed operand, with the gradient's epilogue
static void conv_backward_launch(const DgsConv3x3BackwardDataArgs& g, hipStream_t st) {
    const DgsConv3x3Args a = {g.N, g.H, g.W, g.Cout, g.Cin, g.dy, g.weights, nullptr, 0, g.dx};
    const int Kp = lp_round_up(9 * a.Cin, LP_KC), Cp = lp_round_up(a.Cout, 64);
    const long long M = (long long)a.N * a.H * a.W;
    const bool vec = a.Cin % LP_KC == 0 && lp_aligned16(a.x);
    if (Cp % 128 == 0) {
        const dim3 grid((unsigned)((M + 127) / 128), Cp / 128);
        if (vec) hipLaunchKernelGGL((conv3x3_kernel<2, 2, true, true>), grid, dim3(256), 0, st, a, Cp, Kp, g.mask, g.add);
        else hipLaunchKernelGGL((conv3x3_kernel<2, 2, false, true>), grid, dim3(256), 0, st, a, Cp, Kp, g.mask, g.add);
    } else {
        const dim3 grid((unsigned)((M + 255) / 256), Cp / 64);
        if (vec) hipLaunchKernelGGL((conv3x3_kernel<4, 1, true, true>), grid, dim3(256), 0, st, a, Cp, Kp, g.mask, g.add);
        else hipLaunchKernelGGL((conv3x3_kernel<4, 1, false, true>), grid, dim3(256), 0, st, a, Cp, Kp, g.mask, g.add);
    }
}

static bool conv_backward_ok(const DgsConv3x3BackwardDataArgs* g) {
    if (!g) return false;
    const DgsConv3x3Args a = {g->N, g->H, g->W, g->Cout, g->Cin, g->dy, g->weights, nullptr, 0, g->dx};
    return conv_ok(&a);
}

static bool pool_backward_ok(const DgsMaxPool2x2BackwardArgs* a) {
    return a && a->N >= 1 && a->H >= 1 && a->W >= 1 && a->C >= 1 && a->x && a->dx && (a->dy || a->H == 1 || a->W == 1) &&
           (long long)a->N * a->H * a->W * a->C < (1LL << 40);
}

static void pool_backward_launch(const DgsMaxPool2x2BackwardArgs& a, hipStream_t st) {
    const long long total = (long long)a.N * a.H * a.W * a.C;
    hipLaunchKernelGGL(maxpool2x2_backward_kernel, dim3(lp_blocks(total)), dim3(256), 0, st, a, total);
}

static void tap_backward_launch(const DgsLpipsTapBackwardArgs& a, hipStream_t st) {
    const long long pixels = (long long)a.N * a.H * a.W;
    hipLaunchKernelGGL(lpips_tap_backward_kernel, dim3((unsigned)((pixels + 3) / 4)), dim3(256), 0, st, a, pixels);
}

static void pool_launch(const DgsMaxPool2x2Args& a, hipStream_t st) {
    const long long total = (long long)a.N * (a.H / 2) * (a.W / 2) * a.C;
    if (total > 0) hipLaunchKernelGGL(maxpool2x2_kernel, dim3(lp_blocks(total)), dim3(256), 0, st, a, total);
}

static void tap_launch(const DgsLpipsTapArgs& a, hipStream_t st) {
    const long long pixels = (long long)a.N * a.H * a.W;
    hipLaunchKernelGGL(lpips_tap_pixel_kernel, dim3((unsigned)((pixels + 3) / 4)), dim3(256), 0, st, a, pixels);
    hipLaunchKernelGGL(lpips_tap_mean_kernel, dim3(a.N), dim3(256), 0, st, a);
}

static const int LP_COUT[DGS_LPIPS_CONVS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
static const bool LP_POOL_BEFORE[DGS_LPIPS_CONVS] = {false, false, true, false, true, false, false, true, false, false, true, false, false};
static const int LP_TAP_AFTER[DGS_LPIPS_CONVS] = {-1, 0, -1, 1, -1, -1, 2, -1, -1, 3, -1, -1, 4};

static bool lpips_size_ok(int N, int H, int W) { return N >= 1 && H >= 16 && W >= 16 && (long long)H * W <= (1 << 20); }

struct LpipsWorkspace {
    size_t input, act, pixels, taps;      // floats, each a multiple of 4
    explicit LpipsWorkspace(int cn, int H, int W) {
        const size_t HW = (size_t)H * W;
        input = (2 * (size_t)cn * HW * 3 + 3) / 4 * 4;
        act = 2 * (size_t)cn * HW * 64;   // the largest activation: 64 channels at full size
        pixels = ((size_t)cn * HW + 3) / 4 * 4;
        taps = ((size_t)cn * DGS_LPIPS_TAPS + 3) / 4 * 4;
    }
    size_t bytes() const { return (input + 2 * act + pixels + taps) * sizeof(float); }
};

// the forward's parts, the thirteen ReLU outputs of the chunk's 2 cn images, and two gradient buffers of the largest activation
struct LpipsGradWorkspace {
    LpipsWorkspace f;
    size_t y[DGS_LPIPS_CONVS], kept;      // floats
    int h[DGS_LPIPS_CONVS], w[DGS_LPIPS_CONVS];
    explicit LpipsGradWorkspace(int cn, int H, int W) : f(cn, H, W), kept(0) {
        for (int i = 0; i < DGS_LPIPS_CONVS; ++i) {
            if (LP_POOL_BEFORE[i]) {
                H /= 2;
                W /= 2;
            }
            h[i] = H;
            w[i] = W;
            y[i] = 2 * (size_t)cn * H * W * LP_COUT[i];
            kept += y[i];
        }
    }
    size_t bytes() const { return (f.input + kept + 2 * f.act + f.pixels + f.taps) * sizeof(float); }
};

}  // namespace dgs

extern "C" int64_t dgs_conv3x3_packed_floats(int32_t Cin, int32_t Cout) {
    if (Cin < 1 || Cout < 1 || (long long)Cin * 9 >= (1 << 24) || Cout >= (1 << 24)) return 0;
    return (int64_t)dgs::lp_round_up(9 * Cin, dgs::LP_KC) * dgs::lp_round_up(Cout, 64);
}

extern "C" int dgs_lpips_pack_weights(const DgsLpipsPackArgs* a, dgs_stream_t stream) {
    if (!a || !a->w || !a->packed || dgs_conv3x3_packed_floats(a->Cin, a->Cout) == 0) return DGS_ERR_INVALID_ARGUMENT;
    const int Kp = dgs::lp_round_up(9 * a->Cin, dgs::LP_KC), Cp = dgs::lp_round_up(a->Cout, 64);
    hipLaunchKernelGGL(dgs::lpips_pack_kernel, dim3(dgs::lp_blocks((long long)Kp * Cp)), dim3(256), 0, static_cast<hipStream_t>(stream), *a, Cp, Kp);
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}

extern "C" int dgs_conv3x3(const DgsConv3x3Args* a, dgs_stream_t stream) {
    if (!dgs::conv_ok(a)) return DGS_ERR_INVALID_ARGUMENT;
    dgs::conv_launch(*a, static_cast<hipStream_t>(stream));
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}

extern "C" int dgs_maxpool2x2(const DgsMaxPool2x2Args* a, dgs_stream_t stream) {
    if (!a || a->N < 1 || a->H < 1 || a->W < 1 || a->C < 1 || !a->x || !a->y || (long long)a->N * a->H * a->W * a->C >= (1LL << 40))
        return DGS_ERR_INVALID_ARGUMENT;
    dgs::pool_launch(*a, static_cast<hipStream_t>(stream));
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}

extern "C" int dgs_lpips_tap(const DgsLpipsTapArgs* a, dgs_stream_t stream) {
    if (!a || a->N < 1 || a->H < 1 || a->W < 1 || a->C < 1 || !a->f0 || !a->f1 || !a->lin || !a->out || a->out_stride < 1 || !a->workspace ||
        (long long)a->N * a->H * a->W >= 2147483647LL - 256 || (long long)a->N * a->H * a->W * a->C >= (1LL << 40))
        return DGS_ERR_INVALID_ARGUMENT;
    dgs::tap_launch(*a, static_cast<hipStream_t>(stream));
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}

extern "C" int32_t dgs_lpips_chunk(int32_t N, int32_t H, int32_t W) {
    if (!dgs::lpips_size_ok(N, H, W)) return 0;
    const long long fit = (dgs::LP_PIXEL_BUDGET / 2) / ((long long)H * W);
    return (int32_t)(fit < 1 ? 1 : (fit < N ? fit : N));
}

extern "C" size_t dgs_lpips_workspace_bytes(int32_t N, int32_t H, int32_t W) {
    const int cn = dgs_lpips_chunk(N, H, W);
    return cn ? dgs::LpipsWorkspace(cn, H, W).bytes() : 0;
}

extern "C" int dgs_lpips_forward(const DgsLpipsForwardArgs* a, dgs_stream_t stream) {
    if (!a || !dgs::lpips_size_ok(a->N, a->H, a->W) || !a->x0 || !a->x1 || !a->shift || !a->scale || !a->out || !a->workspace ||
        !dgs::lp_aligned16(a->workspace) || a->chunk < 0)
        return DGS_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < DGS_LPIPS_CONVS; ++i)
        if (!a->conv_w[i] || !a->conv_b[i] || !dgs::lp_aligned16(a->conv_w[i])) return DGS_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < DGS_LPIPS_TAPS; ++k)
        if (!a->lin[k] || (a->features && !a->features[k])) return DGS_ERR_INVALID_ARGUMENT;
    const int largest = dgs_lpips_chunk(a->N, a->H, a->W);
    const int chunk = a->chunk ? a->chunk : largest;
    if (chunk > largest || a->workspace_bytes < dgs::LpipsWorkspace(chunk, a->H, a->W).bytes()) return DGS_ERR_INVALID_ARGUMENT;

    hipStream_t st = static_cast<hipStream_t>(stream);
    const dgs::LpipsWorkspace ws(chunk, a->H, a->W);
    float* input = static_cast<float*>(a->workspace);
    float* act[2] = {input + ws.input, input + ws.input + ws.act};
    float* pixels = act[1] + ws.act;
    float* taps = pixels + ws.pixels;
    const int HW = a->H * a->W;

    for (int first = 0; first < a->N; first += chunk) {
        const int cn = a->N - first < chunk ? a->N - first : chunk;
        hipLaunchKernelGGL(dgs::lpips_input_kernel, dim3(dgs::lp_blocks(2LL * cn * HW)), dim3(256), 0, st, a->x0, a->x1, a->shift, a->scale, first, cn,
                           HW, input);
        const float* cur = input;
        int h = a->H, w = a->W, C = 3, side = 0;
        for (int i = 0; i < DGS_LPIPS_CONVS; ++i) {
            if (dgs::LP_POOL_BEFORE[i]) {
                DgsMaxPool2x2Args p = {2 * cn, h, w, C, cur, act[side]};
                dgs::pool_launch(p, st);
                cur = act[side];
                side ^= 1;
                h /= 2;
                w /= 2;
            }
            DgsConv3x3Args c = {2 * cn, h, w, C, dgs::LP_COUT[i], cur, a->conv_w[i], a->conv_b[i], 1, act[side]};
            dgs::conv_launch(c, st);
            cur = act[side];
            side ^= 1;
            C = dgs::LP_COUT[i];
            const int k = dgs::LP_TAP_AFTER[i];
            if (k < 0) continue;
            const size_t half = (size_t)cn * h * w * C;
            DgsLpipsTapArgs t = {cn, h, w, C, cur, cur + half, a->lin[k], taps + k, DGS_LPIPS_TAPS, pixels};
            dgs::tap_launch(t, st);
            if (a->features) {
                const size_t image = (size_t)h * w * C;
                if (hipMemcpyAsync(a->features[k] + (size_t)first * image, cur, half * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess ||
                    hipMemcpyAsync(a->features[k] + ((size_t)a->N + first) * image, cur + half, half * sizeof(float), hipMemcpyDeviceToDevice, st) !=
                        hipSuccess)
                    return DGS_ERR_DEVICE;
            }
        }
        hipLaunchKernelGGL(dgs::lpips_finish_kernel, dim3(dgs::lp_blocks(cn)), dim3(256), 0, st, taps, cn, a->out + first,
                           a->per_tap ? a->per_tap + (size_t)first * DGS_LPIPS_TAPS : nullptr);
    }
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}

// ---- the input gradient ----

extern "C" int dgs_lpips_pack_weights_transposed(const DgsLpipsPackArgs* a, dgs_stream_t stream) {
    if (!a || !a->w || !a->packed || dgs_conv3x3_packed_floats(a->Cout, a->Cin) == 0) return DGS_ERR_INVALID_ARGUMENT;
    const int Kp = dgs::lp_round_up(9 * a->Cout, dgs::LP_KC), Cp = dgs::lp_round_up(a->Cin, 64);
    hipLaunchKernelGGL(dgs::lpips_pack_transposed_kernel, dim3(dgs::lp_blocks((long long)Kp * Cp)), dim3(256), 0, static_cast<hipStream_t>(stream), *a,
                       Cp, Kp);
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}

extern "C" int dgs_conv3x3_backward_data(const DgsConv3x3BackwardDataArgs* a, dgs_stream_t stream) {
    if (!dgs::conv_backward_ok(a)) return DGS_ERR_INVALID_ARGUMENT;
    dgs::conv_backward_launch(*a, static_cast<hipStream_t>(stream));
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}

extern "C" int dgs_maxpool2x2_backward(const DgsMaxPool2x2BackwardArgs* a, dgs_stream_t stream) {
    if (!dgs::pool_backward_ok(a)) return DGS_ERR_INVALID_ARGUMENT;
    dgs::pool_backward_launch(*a, static_cast<hipStream_t>(stream));
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}

extern "C" int dgs_lpips_tap_backward(const DgsLpipsTapBackwardArgs* a, dgs_stream_t stream) {
    if (!a || a->N < 1 || a->H < 1 || a->W < 1 || a->C < 1 || !a->f0 || !a->f1 || !a->lin || !a->g0 ||
        (long long)a->N * a->H * a->W >= 2147483647LL - 256 || (long long)a->N * a->H * a->W * a->C >= (1LL << 40))
        return DGS_ERR_INVALID_ARGUMENT;
    dgs::tap_backward_launch(*a, static_cast<hipStream_t>(stream));
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}

extern "C" int32_t dgs_lpips_grad_chunk(int32_t N, int32_t H, int32_t W) { return dgs_lpips_chunk(N, H, W); }

extern "C" size_t dgs_lpips_grad_workspace_bytes(int32_t N, int32_t H, int32_t W) {
    const int cn = dgs_lpips_grad_chunk(N, H, W);
    return cn ? dgs::LpipsGradWorkspace(cn, H, W).bytes() : 0;
}

extern "C" int dgs_lpips_forward_backward(const DgsLpipsGradArgs* a, dgs_stream_t stream) {
    if (!a || !dgs::lpips_size_ok(a->N, a->H, a->W) || !a->x0 || !a->x1 || !a->shift || !a->scale || !a->out || !a->grad0 || !a->workspace ||
        !dgs::lp_aligned16(a->workspace) || a->chunk < 0)
        return DGS_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < DGS_LPIPS_CONVS; ++i)
        if (!a->conv_w[i] || !a->conv_wt[i] || !a->conv_b[i] || !dgs::lp_aligned16(a->conv_w[i]) || !dgs::lp_aligned16(a->conv_wt[i]))
            return DGS_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < DGS_LPIPS_TAPS; ++k)
        if (!a->lin[k]) return DGS_ERR_INVALID_ARGUMENT;
    const int largest = dgs_lpips_grad_chunk(a->N, a->H, a->W);
    const int chunk = a->chunk ? a->chunk : largest;
    if (chunk > largest || a->workspace_bytes < dgs::LpipsGradWorkspace(chunk, a->H, a->W).bytes()) return DGS_ERR_INVALID_ARGUMENT;

    hipStream_t st = static_cast<hipStream_t>(stream);
    const dgs::LpipsGradWorkspace ws(chunk, a->H, a->W);
    float* input = static_cast<float*>(a->workspace);
    float* y[DGS_LPIPS_CONVS];
    float* next = input + ws.f.input;
    for (int i = 0; i < DGS_LPIPS_CONVS; ++i) {
        y[i] = next;
        next += ws.y[i];
    }
    float* grad[2] = {next, next + ws.f.act};
    float* pixels = grad[1] + ws.f.act;
    float* taps = pixels + ws.f.pixels;
    const int HW = a->H * a->W;

    for (int first = 0; first < a->N; first += chunk) {
        const int cn = a->N - first < chunk ? a->N - first : chunk;
        // forward, as dgs_lpips_forward runs it, every ReLU output into a buffer of its own (a pool's output into a gradient buffer)
        hipLaunchKernelGGL(dgs::lpips_input_kernel, dim3(dgs::lp_blocks(2LL * cn * HW)), dim3(256), 0, st, a->x0, a->x1, a->shift, a->scale, first, cn,
                           HW, input);
        const float* cur = input;
        int C = 3;
        for (int i = 0; i < DGS_LPIPS_CONVS; ++i) {
            if (dgs::LP_POOL_BEFORE[i]) {
                DgsMaxPool2x2Args p = {2 * cn, ws.h[i - 1], ws.w[i - 1], C, cur, grad[0]};
                dgs::pool_launch(p, st);
                cur = grad[0];
            }
            DgsConv3x3Args c = {2 * cn, ws.h[i], ws.w[i], C, dgs::LP_COUT[i], cur, a->conv_w[i], a->conv_b[i], 1, y[i]};
            dgs::conv_launch(c, st);
            cur = y[i];
            C = dgs::LP_COUT[i];
            const int k = dgs::LP_TAP_AFTER[i];
            if (k < 0) continue;
            DgsLpipsTapArgs t = {cn, ws.h[i], ws.w[i], C, cur, cur + (size_t)cn * ws.h[i] * ws.w[i] * C, a->lin[k], taps + k, DGS_LPIPS_TAPS, pixels};
            dgs::tap_launch(t, st);
        }
        hipLaunchKernelGGL(dgs::lpips_finish_kernel, dim3(dgs::lp_blocks(cn)), dim3(256), 0, st, taps, cn, a->out + first,
                           a->per_tap ? a->per_tap + (size_t)first * DGS_LPIPS_TAPS : nullptr);

        // backward over the first nb images of the chunk: g = dz_i, the gradient at the input of ReLU i
        const int nb = a->grad1 ? 2 * cn : cn;
        float* g = grad[0];
        float* other = grad[1];
        auto tap_backward = [&](int i, float* to) {
            const size_t half = (size_t)cn * ws.h[i] * ws.w[i] * dgs::LP_COUT[i];
            DgsLpipsTapBackwardArgs t = {cn, ws.h[i], ws.w[i], dgs::LP_COUT[i], y[i], y[i] + half, a->lin[dgs::LP_TAP_AFTER[i]], to,
                                         a->grad1 ? to + half : nullptr};
            dgs::tap_backward_launch(t, st);
        };
        tap_backward(DGS_LPIPS_CONVS - 1, g);     // already 0 where y is 0
        for (int i = DGS_LPIPS_CONVS - 1; i >= 1; --i) {
            const bool tap = dgs::LP_TAP_AFTER[i - 1] >= 0;
            if (dgs::LP_POOL_BEFORE[i]) {
                DgsConv3x3BackwardDataArgs c = {nb, ws.h[i], ws.w[i], dgs::LP_COUT[i - 1], dgs::LP_COUT[i], g, a->conv_wt[i], nullptr, nullptr, other};
                dgs::conv_backward_launch(c, st);
                if (tap) tap_backward(i - 1, g);
                DgsMaxPool2x2BackwardArgs p = {nb, ws.h[i - 1], ws.w[i - 1], dgs::LP_COUT[i - 1], y[i - 1], other, 1, tap ? g : nullptr, g};
                dgs::pool_backward_launch(p, st);
            } else {
                if (tap) tap_backward(i - 1, other);
                DgsConv3x3BackwardDataArgs c = {nb, ws.h[i], ws.w[i], dgs::LP_COUT[i - 1], dgs::LP_COUT[i], g, a->conv_wt[i], y[i - 1],
                                                tap ? other : nullptr, other};
                dgs::conv_backward_launch(c, st);
                float* s = g;
                g = other;
                other = s;
            }
        }
        DgsConv3x3BackwardDataArgs c = {nb, a->H, a->W, 3, dgs::LP_COUT[0], g, a->conv_wt[0], nullptr, nullptr, other};
        dgs::conv_backward_launch(c, st);
        hipLaunchKernelGGL(dgs::lpips_input_backward_kernel, dim3(dgs::lp_blocks((long long)nb * HW)), dim3(256), 0, st, other, a->scale, first, cn, nb,
                           HW, a->grad0, a->grad1);
    }
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}
