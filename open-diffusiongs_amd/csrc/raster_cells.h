// raster_cells.h -- the cell-list mechanism of the three blend kernels (blend_forward_kernel, blend_backward_kernel,
// blend_backward_pair_kernel), once.
//
// A tile is sixteen 4 x 4 pixel CELLS.  A batch of 256 entries of the tile's list is staged into LDS (stage_entry), ballots compact it
// into sixteen per-cell index lists (compact_cells), and the lanes that own a cell walk its list, all cells of a wave in lockstep
// (walk_cell).  What a step computes and what a kernel sets up per pixel stay in the kernel.  The kernels declare the LDS arrays (the
// sizes differ per instantiation) and hand them over by reference: after inlining every access is a plain LDS access.
#pragma once
#include "raster_common.h"

namespace dgs {

// A staged entry: pixel position (AUX: (x, y, z, -), the record's xy and p_view.z as one 16-byte word), conic + opacity, colour + the
// alpha cut-off on `power`.
template <bool AUX> using CellXY = typename std::conditional<AUX, float4, float2>::type;
template <bool AUX> struct CellEntry { CellXY<AUX> xy; float4 co; float4 rc; };

// Stages batch entry e: the BlendRecord of Gaussian `id` among the view's `records` (one line per entry, raster_state.h) when the batch
// `has` the entry -- its colour replaced by colors[3 id ..] when colors is given (the backward's colours_precomp of the set) --, else a
// finite zero record: the walk reads ahead of its lists (stale indices), and the product-default arithmetic multiplies a masked-out
// lane's colour by a zero weight instead of selecting -- 0 * NaN from LDS left by an earlier kernel would poison the pixel.  Returns
// the entry's cell_mask (0 without an entry).
template <bool AUX>
__device__ __forceinline__ unsigned stage_entry(bool has, const BlendRecord* records, const float* colors, uint32_t id, int e, float tx0, float ty0,
                                                CellXY<AUX> (&s_xy)[256], float4 (&s_co)[256], float4 (&s_rgbc)[256]) {
    if (!has) {
        if constexpr (AUX) s_xy[e] = make_float4(0.f, 0.f, 0.f, 0.f);
        else s_xy[e] = make_float2(0.f, 0.f);
        s_co[e] = make_float4(0.f, 0.f, 0.f, 0.f); s_rgbc[e] = make_float4(0.f, 0.f, 0.f, 0.f);
        return 0u;
    }
    const BlendRecord* rec = records + id;
    const float4 co = rec->co;
    float4 rc = rec->rc;
    CellXY<AUX> xy;
    if constexpr (AUX) xy = *reinterpret_cast<const float4*>(&rec->xy);     // (x, y, z, -)
    else xy = rec->xy;
    const unsigned m16 = cell_mask(make_float2(xy.x, xy.y), co, rc.w, tx0, ty0);
    if (colors) {
        const float* c = colors + 3 * (size_t)id;
        rc.x = c[0]; rc.y = c[1]; rc.z = c[2];
    }
    s_xy[e] = xy; s_co[e] = co; s_rgbc[e] = rc;
    return m16;
}

// Compacts the staged batch into the per-cell lists: s_list[c] = the batch indices of the entries whose mask has bit c, in batch
// order; s_cnt[c] = how many, per 64 entries of the batch.  A thread staged PARTS entries, entry h * (256 / PARTS) + tid with mask
// m16[h]: one entry per thread of four waves, or two per thread of two waves -- either way the wave's ballot over entry h covers the
// 64 entries number h * (4 / PARTS) + wave of the batch.  Two barriers: counts, then lists (the second also ends the staging).
// One entry per thread keeps its sixteen ballots across the first barrier (32 SGPRs); with two entries they would be 64, so that
// layout ballots again.  Returns the length of `cell`'s list.
template <int PARTS>
__device__ __forceinline__ uint32_t compact_cells(const unsigned (&m16)[PARTS], int cell, int tid, int lane, int wave, unsigned long long lanes_before,
                                                  uint4 (&s_cnt)[16], uint8_t (&s_list)[17][256]) {
    unsigned long long keeps[PARTS][16];
#pragma unroll
    for (int h = 0; h < PARTS; ++h)
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            keeps[h][c] = __ballot((m16[h] >> c) & 1u);
            if (lane == 0) reinterpret_cast<uint32_t*>(&s_cnt[c])[h * (4 / PARTS) + wave] = (uint32_t)__popcll(keeps[h][c]);
        }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < PARTS; ++h)
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const unsigned long long keep = PARTS == 1 ? keeps[h][c] : __ballot((m16[h] >> c) & 1u);
            if ((m16[h] >> c) & 1u) {
                const uint4 cn = s_cnt[c];
                const int part = h * (4 / PARTS) + wave;                // which 64 entries of the batch
                const uint32_t ahead = (part > 0 ? cn.x : 0u) + (part > 1 ? cn.y : 0u) + (part > 2 ? cn.z : 0u);
                s_list[c][ahead + (uint32_t)__popcll(keep & lanes_before)] = (uint8_t)(h * (256 / PARTS) + tid);
            }
        }
    __syncthreads();
    const uint4 cn = s_cnt[cell];
    return cn.x + cn.y + cn.z + cn.w;
}

// Walks a cell's list: step(k, j, entry) for position k = 0, 1, .. of the list, j = the entry's batch index, while more(k) holds
// (tested every four steps, wave-uniform).  Software pipeline: the cell's indices arrive four at a time (one 32-bit word, the next
// word a group ahead), the entry itself (load(j)) one step ahead, in two register sets that take turns -- the loop is unrolled by the
// word, so there is no copy between steps and every shift is a literal (the rotating form spent 13 of the forward's ~45 VALU per step
// on moves).  The walk reads ahead of the list: bytes behind its end are stale indices of earlier batches -- any of them addresses a
// staged record, step has to ignore them (k >= the list's length) --, and the row behind the last cell's is there to be read.
// Returns the k it stopped at.
template <class Load, class Step, class More>
__device__ __forceinline__ uint32_t walk_cell(const uint8_t (&list)[256], const Load& load, const Step& step, const More& more) {
    const uint32_t* lst = reinterpret_cast<const uint32_t*>(list);
    uint32_t word = lst[0];
    auto ea = load(word & 255u);
    decltype(ea) eb;
    uint32_t k = 0;
    for (; more(k); k += 4) {
        const uint32_t word_next = lst[(k >> 2) + 1u];
        eb = load((word >> 8) & 255u);  step(k, word & 255u, ea);
        ea = load((word >> 16) & 255u); step(k + 1u, (word >> 8) & 255u, eb);
        eb = load(word >> 24);          step(k + 2u, (word >> 16) & 255u, ea);
        ea = load(word_next & 255u);    step(k + 3u, word >> 24, eb);
        word = word_next;
    }
    return k;
}

// tile_stats (kRasterStats builds): the tile's walked entries -- `entries` of ONE lane per cell (`counts`) -- and its waves' loop
// trips.  Call with all threads; after the barrier thread 0 has the sums.
template <int WAVES, int N>
__device__ __forceinline__ uint2 tile_stat_sums(bool counts, uint32_t entries, uint32_t trips, int lane, int wave, uint2 (&s_stat)[N]) {
    uint32_t ent = counts ? entries : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ent += (uint32_t)__shfl_xor((int)ent, o);
    if (lane == 0) s_stat[wave] = make_uint2(ent, trips);
    __syncthreads();
    uint2 sum = s_stat[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) { sum.x += s_stat[w].x; sum.y += s_stat[w].y; }
    return sum;
}

// ---- the deterministic backward's epilogue (Params: BwdParams of raster_backward.hip) ----

// Batch entry e when its batch is done: adds the per-wave copies of its NV sums in wave order and STORES them (zeros too) into the
// slot of (Gaussian, this tile) -- Gaussian-major, the tile's index inside the Gaussian's rectangle (the forward's tile_rect on the
// same state: the same rectangle) -- and leaves the copies zero for the next batch.
template <int NV, int NACC, int ROW, class XY, class Params>
__device__ __forceinline__ void store_slots(const Params& p, float (&s_acc)[NACC][NV][ROW], const uint32_t (&s_id)[256], const XY (&s_xy)[256],
                                            int e, bool has, size_t vo, int bx, int by) {
    float c9[NV];
    bool any = false;                                      // any of the per-wave copies non-zero: from the COPIES, not from their sum
#pragma unroll                                             // (partials that cancel exactly would otherwise stay behind for the next batch)
    for (int q = 0; q < NV; ++q) {
        c9[q] = s_acc[0][q][e];
        any = any || c9[q] != 0.f;
#pragma unroll
        for (int w = 1; w < NACC; ++w) {
            const float a = s_acc[w][q][e];
            c9[q] += a;
            any = any || a != 0.f;
        }
    }
    if (!has) return;
    if (any) {
#pragma unroll
        for (int w = 0; w < NACC; ++w)
#pragma unroll
            for (int q = 0; q < NV; ++q) s_acc[w][q][e] = 0.f;
    }
    const size_t gv = vo + s_id[e];
    int x0, y0, x1, y1;
    tile_rect(s_xy[e].x, s_xy[e].y, p.radii[gv], p.gx, p.gy, &x0, &y0, &x1, &y1);
    const size_t slot = (size_t)p.slot_base[gv] + (size_t)((by - y0) * (x1 - x0) + (bx - x0));
    p.slot_a[slot] = make_float4(c9[0], c9[1], c9[2], c9[3]);
    p.slot_b[slot] = make_float4(c9[4], c9[5], c9[6], c9[7]);
    p.slot_c[slot] = c9[8];
    if constexpr (NV > 9) p.slot_d[slot] = c9[9];          // aux calls: dL/dz
}

// What the tile replayed: the first `todo` entries of its list (from `list_begin` in point_list), which is sorted by (depth bits,
// Gaussian index) -- so the key of the deepest one tells which slots the tile wrote.  One thread.
template <class Params>
__device__ __forceinline__ void write_last_key(const Params& p, uint32_t vt, uint32_t list_begin, uint32_t todo, size_t vo) {
    unsigned long long key = 0ull;
    if (todo > 0) {
        const uint32_t id = p.bn.point_list[list_begin + todo - 1u];
        key = ((unsigned long long)__float_as_uint(p.g.depths[vo + id]) << 32) | id;
    }
    p.last_key[vt] = key;
}

// A runtime flag as a template argument: f(std::true_type{}) or f(std::false_type{}).  The launch helpers nest it, one level per flag.
template <class F>
static inline void with_flag(bool flag, const F& f) {
    if (flag) f(std::true_type{});
    else f(std::false_type{});
}

}  // namespace dgs
