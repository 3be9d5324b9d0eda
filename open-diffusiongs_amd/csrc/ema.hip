// ema.hip -- the table-driven EMA launch (include/dgs_ema.h: dgs_ema_plan / dgs_ema_apply).  The fused form lives with the AdamW
// kernel (optim.hip, dgs_adamw_ema_step); this one serves everything else:
//   update, no copies        the EMA update after a step of any other optimizer          8 B read + 4 B written per parameter
//   copies from the shadows  evaluate on the averaged weights: only the engine's bf16 / fp32 / transposed operand copies change
//   copies from p            back to the raw weights                                      4 B read + 2 (+ 2) B written
// Tiling is the AdamW kernel's: a tile is 4,096 consecutive elements of a flat tensor, or a 64 x 64 block of a matrix that also keeps
// a transposed bf16 copy (through LDS once, so that the transposed rows leave as 16-byte stores).  256 threads, 16 bytes per lane and
// access, no atomics, nothing depends on the order of the tiles.
#include "dgs_device.h"
#include "dgs_ema.h"
#include "dit_common.h"
#include "ema_arith.h"

namespace dgs {

template <bool kUpdate, int kSrc>
__global__ __launch_bounds__(256) void ema_apply_kernel(const DgsEmaTensor* __restrict__ tab, int n_tensors, float omd) {
    __shared__ __attribute__((aligned(16))) unsigned short tile[64][64 + 8];     // bf16 block for the transposed copy (rows padded: 144 B)
    const int tid = threadIdx.x, bid = blockIdx.x;
    // the tensor this tile belongs to: the last entry whose first_tile <= bid (uniform: scalar loads)
    int lo = 0, hi = n_tensors - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].first_tile <= bid) lo = mid; else hi = mid - 1;
    }
    const DgsEmaTensor t = tab[lo];
    const int local = bid - t.first_tile;
    // four values: the update when asked for, and what the copies are written from
    auto four = [&](long long i) {
        float4 s;
        if constexpr (kUpdate) {
            const float4 p = *reinterpret_cast<const float4*>(t.p + i);
            float4 e = *reinterpret_cast<const float4*>(t.ema + i);
            e.x = ema_one(e.x, p.x, omd); e.y = ema_one(e.y, p.y, omd); e.z = ema_one(e.z, p.z, omd); e.w = ema_one(e.w, p.w, omd);
            *reinterpret_cast<float4*>(t.ema + i) = e;
            s = kSrc == DGS_EMA_SOURCE_EMA ? e : p;
        } else {
            s = *reinterpret_cast<const float4*>((kSrc == DGS_EMA_SOURCE_EMA ? static_cast<const float*>(t.ema) : t.p) + i);
        }
        return s;
    };
    if (t.copy_t == nullptr) {
        // ---- flat tile: elements [local * 4096, +4096) ----
        const long long n = t.rows * t.cols, base = (long long)local * 4096;
        const bool vec = (n & 3) == 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long i = base + (long long)j * 1024 + tid * 4;
            if (i >= n) break;
            if (vec) {
                const float4 s = four(i);
                if constexpr (kSrc != DGS_EMA_SOURCE_NONE) {
                    if (t.copy_kind == DGS_OPTIM_COPY_BF16)
                        *reinterpret_cast<uint2*>(static_cast<bf16_t*>(t.copy) + i) = make_uint2(pack_bf2(s.x, s.y), pack_bf2(s.z, s.w));
                    else if (t.copy_kind == DGS_OPTIM_COPY_F32) *reinterpret_cast<float4*>(static_cast<float*>(t.copy) + i) = s;
                }
            } else {
                for (int e = 0; e < 4 && i + e < n; ++e) {
                    float s;
                    if constexpr (kUpdate) {
                        const float p = t.p[i + e];
                        const float a = ema_one(t.ema[i + e], p, omd);
                        t.ema[i + e] = a;
                        s = kSrc == DGS_EMA_SOURCE_EMA ? a : p;
                    } else {
                        s = kSrc == DGS_EMA_SOURCE_EMA ? t.ema[i + e] : t.p[i + e];
                    }
                    if constexpr (kSrc != DGS_EMA_SOURCE_NONE) {
                        if (t.copy_kind == DGS_OPTIM_COPY_BF16) static_cast<bf16_t*>(t.copy)[i + e] = (bf16_t)(pack_bf2(s, 0.0f) & 0xffffu);
                        else if (t.copy_kind == DGS_OPTIM_COPY_F32) static_cast<float*>(t.copy)[i + e] = s;
                    }
                }
            }
        }
        return;
    }
    // ---- 64 x 64 block of a matrix with a transposed copy ----
    const int tiles_c = (int)(t.cols / 64);
    const int r0 = (local / tiles_c) * 64, c0 = (local % tiles_c) * 64;
    const int c4 = (tid & 15) * 4, rr = tid >> 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = rr + 16 * j;
        const long long i = (long long)(r0 + r) * t.cols + c0 + c4;
        const float4 s = four(i);
        if constexpr (kSrc != DGS_EMA_SOURCE_NONE) {
            const uint2 b = make_uint2(pack_bf2(s.x, s.y), pack_bf2(s.z, s.w));
            if (t.copy_kind == DGS_OPTIM_COPY_BF16) *reinterpret_cast<uint2*>(static_cast<bf16_t*>(t.copy) + i) = b;
            else if (t.copy_kind == DGS_OPTIM_COPY_F32) *reinterpret_cast<float4*>(static_cast<float*>(t.copy) + i) = s;
            *reinterpret_cast<uint2*>(&tile[r][c4]) = b;
        }
    }
    if constexpr (kSrc != DGS_EMA_SOURCE_NONE) {
        __syncthreads();
        // transposed: thread -> column c of the block, 16 consecutive rows: 32 contiguous bytes of copy_t[c0 + c][r0 + ...]
        const int c = tid >> 2, rq = (tid & 3) * 16;
        unsigned short u[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) u[e] = tile[rq + e][c];
        bf16_t* dst = static_cast<bf16_t*>(t.copy_t) + (long long)(c0 + c) * t.rows + r0 + rq;
        auto pk = [&](int e) { return (uint32_t)u[e] | ((uint32_t)u[e + 1] << 16); };
        *reinterpret_cast<uint4*>(dst) = make_uint4(pk(0), pk(2), pk(4), pk(6));
        *reinterpret_cast<uint4*>(dst + 8) = make_uint4(pk(8), pk(10), pk(12), pk(14));
    }
}

template <bool kUpdate, int kSrc>
static void launch(const DgsEmaArgs* a, hipStream_t stream) {
    hipLaunchKernelGGL((ema_apply_kernel<kUpdate, kSrc>), dim3(a->n_tiles), dim3(256), 0, stream, a->tensors, a->n_tensors, a->one_minus_decay);
}

}  // namespace dgs

extern "C" int32_t dgs_ema_plan(DgsEmaTensor* tab, int32_t n) {
    if (!tab || n <= 0) return -1;
    long long tiles = 0;
    for (int i = 0; i < n; ++i) {
        DgsEmaTensor& t = tab[i];
        if (!t.p || !t.ema || t.rows <= 0 || t.cols <= 0) return -1;
        // the kernel moves 16 bytes per lane (8 for a bf16 copy): a tensor that is a view at an odd element offset has no such alignment
        const auto misaligned = [](const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; };
        if (misaligned(t.p, 16) || misaligned(t.ema, 16)) return -1;
        if (t.copy && misaligned(t.copy, t.copy_kind == DGS_OPTIM_COPY_BF16 ? 8 : 16)) return -1;
        if (t.copy_t && misaligned(t.copy_t, 16)) return -1;
        if (t.copy_kind < DGS_OPTIM_COPY_NONE || t.copy_kind > DGS_OPTIM_COPY_F32 || (t.copy_kind != DGS_OPTIM_COPY_NONE && !t.copy)) return -1;
        t.first_tile = (int32_t)tiles;
        if (t.copy_t) {
            if (t.rows % 64 || t.cols % 64) return -1;
            tiles += (t.rows / 64) * (t.cols / 64);
        } else {
            tiles += (t.rows * t.cols + 4095) / 4096;
        }
        if (tiles > 0x7fffffffLL) return -1;
    }
    return (int32_t)tiles;
}

extern "C" int dgs_ema_apply(const DgsEmaArgs* a, dgs_stream_t stream) {
    if (!a || !a->tensors || a->n_tensors <= 0 || a->n_tiles <= 0) return DGS_ERR_INVALID_ARGUMENT;
    if (a->copy_source < DGS_EMA_SOURCE_NONE || a->copy_source > DGS_EMA_SOURCE_EMA) return DGS_ERR_INVALID_ARGUMENT;
    if (!a->update && a->copy_source == DGS_EMA_SOURCE_NONE) return DGS_ERR_INVALID_ARGUMENT;
    if (a->update && !(a->one_minus_decay >= 0.0f && a->one_minus_decay <= 1.0f)) return DGS_ERR_INVALID_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a->update) {
        if (a->copy_source == DGS_EMA_SOURCE_NONE) dgs::launch<true, DGS_EMA_SOURCE_NONE>(a, s);
        else if (a->copy_source == DGS_EMA_SOURCE_P) dgs::launch<true, DGS_EMA_SOURCE_P>(a, s);
        else dgs::launch<true, DGS_EMA_SOURCE_EMA>(a, s);
    } else {
        if (a->copy_source == DGS_EMA_SOURCE_P) dgs::launch<false, DGS_EMA_SOURCE_P>(a, s);
        else dgs::launch<false, DGS_EMA_SOURCE_EMA>(a, s);
    }
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}
