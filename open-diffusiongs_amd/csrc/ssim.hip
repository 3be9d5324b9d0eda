// ssim.hip -- SSIM (11-tap Gaussian window, sigma 1.5, VALID) forward and backward fused with the MSE term (include/dgs_loss.h
// DgsSsimArgs; the reference's SsimLoss, diffusionGS/utils/losses.py:216-234, evaluated over all b * v views, :317-321).
//
// A workgroup of 256 threads owns a tile of 64 x 16 pixels of one image plane.
//   forward   stage x and y of the tile + halo of 10 (74 x 26, row pitch 76) in LDS once; horizontal pass: the five rows
//             G_w(x), G_w(y), G_w(x x), G_w(y y), G_w(x y) (26 x 64 each) into LDS, a thread owning four neighbouring columns of a row
//             (16 staged values of x and y read as float4, every product formed once, 4 x 11 taps in registers); vertical pass: a thread
//             owns one column and four rows, 14 LDS reads per map feed 4 x 11 taps, straight into the per-pixel expression.  No
//             moment map goes to memory.  Tile sums of m and of (x - y)^2 (every input pixel is owned by exactly one tile) are reduced in
//             a fixed tree and written to the workspace; ssim_final_kernel adds them in index order.  With `saved` the three
//             partial-derivative maps a = p_mu - 2 mu1 p_s1 - mu2 p_s12, p_s1, p_s12 are stored.
//   backward  a gather, the same two passes over the three saved maps, zero-extended by 10:
//             dx(p) = g[n] / (C (H-10)(W-10)) (Gt(a) + 2 x Gt(p_s1) + y Gt(p_s12))(p) + mse_scale[b] 2 (x - y)(p) / (V C H W); one store,
//             no atomics.
// LDS: the vertical pass reads ds_read_b32 with consecutive lanes on consecutive columns, the horizontal pass ds_read_b128 with
// consecutive lanes on consecutive 16-byte slots (both conflict-free by the bank rules); global staging is 16 bytes per lane when
// W % 4 == 0 and the bases are 16-byte aligned (a tile starts at a multiple of 64 columns), scalar otherwise.
// The saved maps keep the input's plane geometry, element (oy, ox) at [oy][ox + 2]: the backward's window starts at ox = x0 - 10,
// i.e. at column x0 - 8, a multiple of 4, and 16-byte loads work there too.  Cells outside the (H-10) x (W-10) map are never
// written; the backward's staging zeroes them by coordinate.
// Taps accumulate with explicit fmaf (v_fma_f32 / v_pk_fma_f32 on the device, the host's FMA in the emulator build: same bits);
// everything else is un-fused (-ffp-contract=off, dgs_amd/build.py STRICT_FP), so the emulator build and the device round alike.
//
// Traffic and arithmetic, b = 4, v = 10, 256^2 (one f32 image tensor P = 31.5 MB; unique bytes, halo re-reads are cache hits):
//   forward only                       reads x, y                                                   63 MB
//   save maps (this file)   forward    reads x, y; writes a, p_s1, p_s12 (3 x 29 MB of 246^2 maps)  150 MB
//                           backward   reads the 3 maps, x, y; writes dx                            182 MB     total 332 MB
//   recompute               forward    reads x, y                                                   63 MB
//                           backward   reads x, y; writes dx                                        94 MB      total 157 MB
//   filter arithmetic per output pixel (multiply / FMA lanes, the halo rows of the horizontal pass included): forward
//   (14 x 3 / 4 + 11 x 5) x 26/16 + 11 x 5 = 161, backward over saved maps 11 x 3 x 26/16 + 11 x 3 = 87; a recomputing backward
//   filters the five moments over a tile with a halo of 20 ((10.5 + 55) x 36/16 x 84/64 + 55 x 26/16 x 74/64 = 297) before the same
//   87: about 2.5 times the filter arithmetic of forward + backward here for 47 % of the bytes.
//   Measured (MI355X, rocprofv3 kernel trace, profiles/ssim_kernel_stats.txt): forward 91 us, backward 79 us, finish 5 us at
//   40 x 3 x 256^2; 415 / 372 / 20 us at 44 x 3 x 512^2: 1.85 TB/s, 29 % of the 6.29 TB/s copy bandwidth.  Both kernels are bound by
//   VALU issue and by occupancy (3 workgroups per CU, LDS), not by HBM, so the recomputing form -- fewer bytes, more than twice the
//   arithmetic -- has nothing to gain here; it was not built, and only the save-maps form is measured.
//
// Deterministic: fixed tap order, fixed tree inside the workgroup, tile sums in index order.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), no scratch anywhere:
//   ssim_forward_kernel<vec / scalar>    94 / 96 VGPRs, 68 SGPRs, 50,112 B LDS, 3 waves per SIMD
//   ssim_backward_kernel<vec / scalar>   96 / 96 VGPRs, 103 SGPRs, 43,680 B LDS, 3 waves per SIMD
//   ssim_final_kernel                    22 VGPRs, 42 SGPRs, no LDS
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "dgs_loss.h"

namespace dgs {

constexpr int SSIM_WIN = 11, SSIM_HALO = SSIM_WIN - 1;
constexpr int SSIM_TW = 64, SSIM_TH = 16;                                   // output tile
constexpr int SSIM_SW = SSIM_TW + SSIM_HALO, SSIM_SH = SSIM_TH + SSIM_HALO; // staged tile 74 x 26
constexpr int SSIM_SP = 76;                                                 // staged row pitch (19 float4)
constexpr int SSIM_ROWS = 4;                                                // output rows per thread in the vertical pass

struct SsimWindow { float w[SSIM_WIN]; };

struct SsimGeom {
    int oh, ow, tiles_x, tiles_y;
    __host__ __device__ SsimGeom(int H, int W, bool backward) : oh(H - SSIM_HALO), ow(W - SSIM_HALO) {
        tiles_x = ((backward ? W : ow) + SSIM_TW - 1) / SSIM_TW;
        tiles_y = ((backward ? H : oh) + SSIM_TH - 1) / SSIM_TH;
    }
};

__device__ __forceinline__ float ssim_block_sum(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// Stage rows [y0, y0 + 26) x columns [x0, x0 + 76) of a plane with `pitch` columns into LDS (pitch SSIM_SP).  Cells outside
// rows [0, rows) or columns [clo, chi) (0 <= clo, chi <= pitch) become zero whatever memory holds there.  On the vector path x0 and
// pitch are multiples of 4 (x0 may be negative), so a group of four columns is entirely inside or entirely outside the plane's row.
template <bool VEC>
__device__ __forceinline__ void ssim_stage(float* dst, const float* plane, int y0, int x0, int rows, int pitch, int clo, int chi) {
    if (VEC) {
        for (int i = threadIdx.x; i < SSIM_SH * (SSIM_SP / 4); i += 256) {
            const int r = i / (SSIM_SP / 4), j = i - r * (SSIM_SP / 4);
            const int gy = y0 + r, gx = x0 + 4 * j;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gy >= 0 && gy < rows && gx >= 0 && gx < pitch) v = *reinterpret_cast<const float4*>(plane + (size_t)gy * pitch + gx);
            v.x = (gx >= clo && gx < chi) ? v.x : 0.f;
            v.y = (gx + 1 >= clo && gx + 1 < chi) ? v.y : 0.f;
            v.z = (gx + 2 >= clo && gx + 2 < chi) ? v.z : 0.f;
            v.w = (gx + 3 >= clo && gx + 3 < chi) ? v.w : 0.f;
            *reinterpret_cast<float4*>(dst + r * SSIM_SP + 4 * j) = v;
        }
    } else {
        for (int i = threadIdx.x; i < SSIM_SH * SSIM_SP; i += 256) {
            const int r = i / SSIM_SP, c = i - r * SSIM_SP;
            const int gy = y0 + r, gx = x0 + c;
            dst[i] = (gy >= 0 && gy < rows && gx >= clo && gx < chi) ? plane[(size_t)gy * pitch + gx] : 0.f;
        }
    }
}

// Vertical pass: out[m][o] = sum_k w[k] h[m][(r0 + o + k) * 64 + c], o = 0 .. 3; each of the 14 rows is read once.
template <int NM>
__device__ __forceinline__ void ssim_vpass(const float* h, const SsimWindow& win, int r0, int c, float (&out)[NM][SSIM_ROWS]) {
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int o = 0; o < SSIM_ROWS; ++o) out[m][o] = 0.f;
#pragma unroll
    for (int rr = 0; rr < SSIM_ROWS + SSIM_HALO; ++rr) {
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const float v = h[m * (SSIM_SH * SSIM_TW) + (r0 + rr) * SSIM_TW + c];
#pragma unroll
            for (int o = 0; o < SSIM_ROWS; ++o)
                if (rr - o >= 0 && rr - o < SSIM_WIN) out[m][o] = fmaf(win.w[rr - o], v, out[m][o]);
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void ssim_forward_kernel(DgsSsimArgs a, SsimWindow win) {
    __shared__ __attribute__((aligned(16))) float sx[SSIM_SH * SSIM_SP];
    __shared__ __attribute__((aligned(16))) float sy[SSIM_SH * SSIM_SP];
    __shared__ __attribute__((aligned(16))) float hm[5 * SSIM_SH * SSIM_TW];
    __shared__ float red[256];
    const SsimGeom g(a.H, a.W, false);
    const int plane = blockIdx.z, x0 = blockIdx.x * SSIM_TW, y0 = blockIdx.y * SSIM_TH;
    const size_t HW = (size_t)a.H * a.W;
    ssim_stage<VEC>(sx, a.x + plane * HW, y0, x0, a.H, a.W, 0, a.W);
    ssim_stage<VEC>(sy, a.y + plane * HW, y0, x0, a.H, a.W, 0, a.W);
    __syncthreads();

    // squared error of the input pixels this tile owns: its 64 x 16 cells, the last tile of a row / column also the 10 beyond
    float sq = 0.f;
    if (a.l2) {
        const int cw = (int)blockIdx.x == g.tiles_x - 1 ? a.W - x0 : SSIM_TW, rh = (int)blockIdx.y == g.tiles_y - 1 ? a.H - y0 : SSIM_TH;
        for (int i = threadIdx.x; i < SSIM_SH * (SSIM_SP / 4); i += 256) {
            const int r = i / (SSIM_SP / 4), c = 4 * (i - r * (SSIM_SP / 4));
            const float4 xv = *reinterpret_cast<const float4*>(sx + r * SSIM_SP + c), yv = *reinterpret_cast<const float4*>(sy + r * SSIM_SP + c);
            const float d0 = xv.x - yv.x, d1 = xv.y - yv.y, d2 = xv.z - yv.z, d3 = xv.w - yv.w;
            if (r < rh) {
                sq += c < cw ? d0 * d0 : 0.f;
                sq += c + 1 < cw ? d1 * d1 : 0.f;
                sq += c + 2 < cw ? d2 * d2 : 0.f;
                sq += c + 3 < cw ? d3 * d3 : 0.f;
            }
        }
    }

    // horizontal pass: a thread owns four neighbouring columns of one row, reads its 16 staged values of x and y as float4 and forms
    // every product once; the 4 x 11 taps run in registers
    for (int i = threadIdx.x; i < SSIM_SH * (SSIM_TW / 4); i += 256) {
        const int r = i / (SSIM_TW / 4), c = 4 * (i - r * (SSIM_TW / 4));
        float xv[16], yv[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 u = *reinterpret_cast<const float4*>(sx + r * SSIM_SP + c + 4 * q), v = *reinterpret_cast<const float4*>(sy + r * SSIM_SP + c + 4 * q);
            xv[4 * q] = u.x; xv[4 * q + 1] = u.y; xv[4 * q + 2] = u.z; xv[4 * q + 3] = u.w;
            yv[4 * q] = v.x; yv[4 * q + 1] = v.y; yv[4 * q + 2] = v.z; yv[4 * q + 3] = v.w;
        }
        float m1[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f}, xx[4] = {0.f, 0.f, 0.f, 0.f}, yy[4] = {0.f, 0.f, 0.f, 0.f}, xy[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4 + SSIM_HALO; ++t) {
            const float px = xv[t] * xv[t], py = yv[t] * yv[t], pxy = xv[t] * yv[t];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (t - j >= 0 && t - j < SSIM_WIN) {
                    const float w = win.w[t - j];
                    m1[j] = fmaf(w, xv[t], m1[j]);
                    m2[j] = fmaf(w, yv[t], m2[j]);
                    xx[j] = fmaf(w, px, xx[j]);
                    yy[j] = fmaf(w, py, yy[j]);
                    xy[j] = fmaf(w, pxy, xy[j]);
                }
        }
        const int at = r * SSIM_TW + c;
        *reinterpret_cast<float4*>(hm + at) = make_float4(m1[0], m1[1], m1[2], m1[3]);
        *reinterpret_cast<float4*>(hm + SSIM_SH * SSIM_TW + at) = make_float4(m2[0], m2[1], m2[2], m2[3]);
        *reinterpret_cast<float4*>(hm + 2 * SSIM_SH * SSIM_TW + at) = make_float4(xx[0], xx[1], xx[2], xx[3]);
        *reinterpret_cast<float4*>(hm + 3 * SSIM_SH * SSIM_TW + at) = make_float4(yy[0], yy[1], yy[2], yy[3]);
        *reinterpret_cast<float4*>(hm + 4 * SSIM_SH * SSIM_TW + at) = make_float4(xy[0], xy[1], xy[2], xy[3]);
    }
    __syncthreads();

    const int c = threadIdx.x & (SSIM_TW - 1), r0 = (threadIdx.x / SSIM_TW) * SSIM_ROWS;
    float f[5][SSIM_ROWS];
    ssim_vpass<5>(hm, win, r0, c, f);
    const float C1 = (0.01f * a.data_range) * (0.01f * a.data_range), C2 = (0.03f * a.data_range) * (0.03f * a.data_range);
    const int ox = x0 + c;
    float* sv = a.saved ? a.saved + plane * HW : nullptr;
    const size_t map = (size_t)a.N * a.C * HW;
    float acc = 0.f;
#pragma unroll
    for (int o = 0; o < SSIM_ROWS; ++o) {
        const int oy = y0 + r0 + o;
        const float mu1 = f[0][o], mu2 = f[1][o];
        const float s1 = f[2][o] - mu1 * mu1, s2 = f[3][o] - mu2 * mu2, s12 = f[4][o] - mu1 * mu2;
        const float A = 2.f * (mu1 * mu2) + C1, B = (mu1 * mu1 + mu2 * mu2) + C1, Cn = 2.f * s12 + C2, D = (s1 + s2) + C2;
        const float rB = 1.0f / B, rD = 1.0f / D;             // two correctly rounded divisions per pixel; the rest are products
        const float ab = A * rB, cd = Cn * rD;
        if (oy < g.oh && ox < g.ow) {
            acc += ab * cd;
            if (sv) {
                const float p_mu = (2.f * mu2 * B - 2.f * mu1 * A) * (rB * rB) * cd;
                const float p_s1 = -(ab * cd) * rD, p_s12 = 2.f * ab * rD;
                const size_t at = (size_t)oy * a.W + ox + 2;
                sv[at] = p_mu - 2.f * mu1 * p_s1 - mu2 * p_s12;
                sv[map + at] = p_s1;
                sv[2 * map + at] = p_s12;
            }
        }
    }
    acc = ssim_block_sum(acc, red);
    if (a.l2) sq = ssim_block_sum(sq, red);
    if (threadIdx.x == 0) {
        float* p = a.workspace + 2 * (((size_t)plane * g.tiles_y + blockIdx.y) * g.tiles_x + blockIdx.x);
        p[0] = acc;
        p[1] = sq;
    }
}

// One workgroup per sample, a wave per image (images w, w + 4, ... of the sample): lane-strided sums of the image's C * tiles tile
// sums in index order, a fixed butterfly across the lanes; then thread 0 adds the images' squared-error sums in index order.
__global__ __launch_bounds__(256) void ssim_final_kernel(DgsSsimArgs a) {
    const SsimGeom g(a.H, a.W, false);
    const int b = blockIdx.x, V = a.N / a.B, per = a.C * g.tiles_x * g.tiles_y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv = 1.0f / ((float)a.C * (float)g.oh * (float)g.ow);
    float* sq_image = a.workspace + 2 * (size_t)a.N * per;
    for (int v = wave; v < V; v += 4) {
        const int n = b * V + v;
        const float* p = a.workspace + 2 * (size_t)n * per;
        float s = 0.f, q = 0.f;
        for (int i = lane; i < per; i += 64) { s += p[2 * i]; q += p[2 * i + 1]; }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) { s += __shfl_xor(s, m); q += __shfl_xor(q, m); }
        if (lane == 0) { a.ssim[n] = s * inv; sq_image[n] = q; }
    }
    if (!a.l2) return;
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
        float total = 0.f;
        for (int v = 0; v < V; ++v) total += sq_image[b * V + v];
        const float l2 = total / ((float)V * (float)a.C * (float)a.H * (float)a.W);
        a.l2[b] = l2;
        if (a.psnr) a.psnr[b] = -10.0f * log10f(l2);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void ssim_backward_kernel(DgsSsimArgs a, SsimWindow win) {
    __shared__ __attribute__((aligned(16))) float sm[3 * SSIM_SH * SSIM_SP];
    __shared__ __attribute__((aligned(16))) float hm[3 * SSIM_SH * SSIM_TW];
    const SsimGeom g(a.H, a.W, true);
    const int plane = blockIdx.z, x0 = blockIdx.x * SSIM_TW, y0 = blockIdx.y * SSIM_TH;
    const size_t HW = (size_t)a.H * a.W, map = (size_t)a.N * a.C * HW;
    // this thread's four pixels of x and y: requested first, used last (their latency hides behind the staging and the two passes)
    const int c = threadIdx.x & (SSIM_TW - 1), r0 = (threadIdx.x / SSIM_TW) * SSIM_ROWS, px = x0 + c;
    float xv[SSIM_ROWS], yv[SSIM_ROWS];
#pragma unroll
    for (int o = 0; o < SSIM_ROWS; ++o) {
        const int py = y0 + r0 + o;
        const bool in = py < a.H && px < a.W;
        xv[o] = in ? a.x[plane * HW + (size_t)py * a.W + px] : 0.f;
        yv[o] = in ? a.y[plane * HW + (size_t)py * a.W + px] : 0.f;
    }
    // map rows [y0 - 10, y0 + 16), map columns [x0 - 10, x0 + 66) = stored columns [x0 - 8, x0 + 68); what lies outside the map (stored
    // columns [2, ow + 2), rows [0, oh)) was never written and is staged as zero: the zero extension of Gt
#pragma unroll
    for (int m = 0; m < 3; ++m)
        ssim_stage<VEC>(sm + m * SSIM_SH * SSIM_SP, a.saved + m * map + plane * HW, y0 - SSIM_HALO, x0 - SSIM_HALO + 2, g.oh, a.W, 2, g.ow + 2);
    __syncthreads();

    // horizontal pass, four columns per thread as in the forward; staged column c4 + t is map column x0 - 10 + c4 + t
    for (int i = threadIdx.x; i < SSIM_SH * (SSIM_TW / 4); i += 256) {
        const int r = i / (SSIM_TW / 4), c4 = 4 * (i - r * (SSIM_TW / 4));
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            float v[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 u = *reinterpret_cast<const float4*>(sm + m * SSIM_SH * SSIM_SP + r * SSIM_SP + c4 + 4 * q);
                v[4 * q] = u.x; v[4 * q + 1] = u.y; v[4 * q + 2] = u.z; v[4 * q + 3] = u.w;
            }
            float h[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 4 + SSIM_HALO; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (t - j >= 0 && t - j < SSIM_WIN) h[j] = fmaf(win.w[SSIM_HALO - (t - j)], v[t], h[j]);
            *reinterpret_cast<float4*>(hm + m * SSIM_SH * SSIM_TW + r * SSIM_TW + c4) = make_float4(h[0], h[1], h[2], h[3]);
        }
    }
    __syncthreads();

    float f[3][SSIM_ROWS];
    ssim_vpass<3>(hm, win, r0, c, f);
    const int n = plane / a.C, V = a.N / a.B, b = n / V;
    const float gs = a.g[n] / ((float)a.C * (float)g.oh * (float)g.ow);
    const float ms = a.mse_scale ? a.mse_scale[b] * 2.0f / ((float)V * (float)a.C * (float)a.H * (float)a.W) : 0.f;
#pragma unroll
    for (int o = 0; o < SSIM_ROWS; ++o) {
        const int py = y0 + r0 + o;
        if (py < a.H && px < a.W)
            a.dx[plane * HW + (size_t)py * a.W + px] = gs * ((f[0][o] + 2.f * xv[o] * f[1][o]) + yv[o] * f[2][o]) + ms * (xv[o] - yv[o]);
    }
}

// w[k] = exp(-(k - 5)^2 / (2 * 1.5^2)) / sum, evaluated and normalised in fp32 the way the library builds its window with torch
// (arange, exp, sum, divide); kept as literals so that the window does not depend on the host's libm (1 ulp on a few taps moves
// ssim by ~3e-7).  Symmetric; the fp32 sum is 1 - 3e-8.
static SsimWindow ssim_window() {
    const float half[6] = {0x1.0d957p-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f};
    SsimWindow win;
    for (int k = 0; k < SSIM_WIN; ++k) win.w[k] = half[k < 6 ? k : SSIM_WIN - 1 - k];
    return win;
}

static bool ssim_shape_ok(const DgsSsimArgs* a) {
    return a && a->N > 0 && a->C > 0 && a->H >= SSIM_WIN && a->W >= SSIM_WIN && a->B > 0 && a->N % a->B == 0 && (long long)a->N * a->C <= 65535 &&
           a->x && a->y;
}

static bool ssim_aligned(const DgsSsimArgs* a, const void* third) {
    return a->W % 4 == 0 && (((uintptr_t)a->x | (uintptr_t)a->y | (uintptr_t)third) & 15) == 0;
}

}  // namespace dgs

extern "C" int64_t dgs_ssim_workspace_floats(int32_t N, int32_t C, int32_t H, int32_t W) {
    if (N <= 0 || C <= 0 || H < dgs::SSIM_WIN || W < dgs::SSIM_WIN) return 0;
    const dgs::SsimGeom g(H, W, false);
    return 2 * (int64_t)N * C * g.tiles_x * g.tiles_y + N;            // (m, squared error) per tile | squared error per image
}

extern "C" int64_t dgs_ssim_saved_floats(int32_t N, int32_t C, int32_t H, int32_t W) {
    if (N <= 0 || C <= 0 || H < dgs::SSIM_WIN || W < dgs::SSIM_WIN) return 0;
    return 3 * (int64_t)N * C * H * W;
}

extern "C" int dgs_ssim(const DgsSsimArgs* a, dgs_stream_t stream) {
    if (!dgs::ssim_shape_ok(a) || !a->ssim || !a->workspace || (a->psnr && !a->l2)) return DGS_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dgs::SsimGeom g(a->H, a->W, false);
    const dgs::SsimWindow win = dgs::ssim_window();
    const dim3 grid(g.tiles_x, g.tiles_y, a->N * a->C);
    if (dgs::ssim_aligned(a, a->saved))
        hipLaunchKernelGGL(dgs::ssim_forward_kernel<true>, grid, dim3(256), 0, st, *a, win);
    else
        hipLaunchKernelGGL(dgs::ssim_forward_kernel<false>, grid, dim3(256), 0, st, *a, win);
    hipLaunchKernelGGL(dgs::ssim_final_kernel, dim3(a->B), dim3(256), 0, st, *a);
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}

extern "C" int dgs_ssim_backward(const DgsSsimArgs* a, dgs_stream_t stream) {
    if (!dgs::ssim_shape_ok(a) || !a->saved || !a->g || !a->dx) return DGS_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dgs::SsimGeom g(a->H, a->W, true);
    const dgs::SsimWindow win = dgs::ssim_window();
    const dim3 grid(g.tiles_x, g.tiles_y, a->N * a->C);
    if (dgs::ssim_aligned(a, a->saved))
        hipLaunchKernelGGL(dgs::ssim_backward_kernel<true>, grid, dim3(256), 0, st, *a, win);
    else
        hipLaunchKernelGGL(dgs::ssim_backward_kernel<false>, grid, dim3(256), 0, st, *a, win);
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}
