// mesh_decimate.hip -- vertex clustering of a triangle mesh on a uniform grid of n cells per axis, on the device
// (include/dgs_mesh_decimate.h DgsMeshDecimateArgs; the order-free counterpart of the reference's decimate_mesh, MeshLab's
// meshing_decimation_clustering followed by the removal of null and duplicate faces).  The header holds the definition; this file is its
// kernel sequence.
//
// dgs_mesh_decimate_count (two memsets: the zeroed arrays, the table of face indices to 0xff):
//   dec_ref_kernel        thread = face: validity (invalid faces counted, one atomic a wave), ref[a] = ref[b] = ref[c] = 1.
//   dec_box_kernel        thread = vertex: the box of the referenced vertices as clean_box_kernel takes the mesh's: atomicMax of the
//                         order-preserving uint32 image of the floats (minima stored complemented), combined over the wave and the
//                         workgroup first and issued only when the word read first is lower.
//   dec_params_kernel     one wave: lo as doubles, ext, inv = n / ext, n - 1, and the EMPTY flag (no valid face, or ext not above 0);
//                         every kernel behind it returns at once when the flag is set.  Every fp64 operand comes from a per-lane load
//                         (csrc/mesh_clean.hip, clean_threshold_kernel, says why) and n arrives as a double.
//   dec_cell_kernel       thread = vertex: the cell of a referenced vertex in fp64 (dec_locate), kept in vrank[v], and its bit in a mask
//                         of n^3 bits: atomicOr, after an atomic load that shows the bit missing.  128 MiB at n = 1024, 2 MiB at 256.
//   dec_occ_kernel        thread = 512 bits of the mask (eight 64-bit words, one 64-byte piece): population count, exclusive scan over
//                         the workgroup, block totals aside.
//   dec_occ_sums_kernel   one workgroup: exclusive scan of the block totals.
//   dec_rank_kernel       thread = vertex: vrank[v] = the rank of its cell among the occupied cells = block prefix + piece prefix + the
//                         population count of the bits below it in its piece (at most eight words of one 64-byte line); cellof[rank].
//   dec_insert_kernel     thread = face: the ranks of its corners; two equal: degenerate, no slot.  Otherwise it goes into
//                         an open-addressing table of face indices with at least 2 F slots: atomicCAS(slot, EMPTY, f); a slot
//                         that holds a face of the same three ranks takes atomicMin(slot, f); any other occupant: the next slot.  The
//                         occupant's ranks are read from faces[] and vrank[], which nothing writes in this launch; the table itself is
//                         only touched by atomics (the XCDs' L2s are not coherent for plain loads inside a launch).  The slots a key
//                         passes are taken for good, so all faces of one key end in one slot, which finally holds their smallest
//                         index whichever came first.  The probe loop is bounded by the capacity and never waits; a probe that found no
//                         slot (impossible while the table has more slots than faces) sets the error word.
//   dec_fscan_kernel      thread = face, the next launch: kept iff its slot holds its own index; exclusive scan, block totals aside;
//                         used[rank] = 1 for the corners of a kept face (the same value from every writer).  The faces that have a
//                         slot at all ride in the upper half of the scanned word: the degenerate ones are what is left of the valid
//                         ones.  (Counted with one atomicAdd a wave in the inserting launch, 24,000 adds on one address, that launch
//                         took 286 us at 1.57 M faces whatever n: atomics of one address are served one after another.)
//   dec_uscan_kernel      thread = rank: exclusive scan of used[].
//   dec_sums_kernel       one workgroup: exclusive scan of both lists of block totals, the five counts to the caller.
// dgs_mesh_decimate_emit (one memset: the accumulators):
//   dec_accumulate_kernel thread = vertex: a referenced vertex of a used cluster adds 1 to count[rank] and its three fixed-point
//                         offsets (dec_locate again: the same instructions, the same bits) to sum[rank]: integer atomicAdd, 32 and 64 bit.
//   dec_emit_vertices_kernel  thread = rank: a used cluster's position (the header's fp64 expression) to block base + offset.
//   dec_emit_faces_kernel thread = face: a kept face to block base + offset, its corners renumbered through the clusters' offsets.
// Only the emit call needs the accumulators, so a caller that bisects n (consumers.decimate_mesh) pays for them once.
// The only atomics are the or, the integer adds and the table's compare-and-swap / minimum; positions come from the scans.  Same input,
// same bytes.  STRICT_FP (dgs_amd/build.py): no fused multiply-add, so numpy (tests/mesh_decimate_util.py) and the emulator build
// compute every cell, offset and position as the device does.
//
// Workspace: 8 B a vertex, 8 B a face, 8-16 B a face for the table, 40 B per possible cluster (min(V, n^3)), n^3 / 8 B of mask and a
// sixteenth of that for its prefixes.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "dgs_device.h"
#include "dgs_mesh_decimate.h"
#include "mesh_common.h"

namespace dgs {

constexpr int DEC_WG = 256;
constexpr int64_t DEC_MAX_ROWS = (int64_t)1 << 30;
constexpr int DEC_MAX_N = 1024;
constexpr uint32_t DEC_NONE = 0xffffffffu;           // no face index, no slot: F <= 2^30, slots < 2^31
constexpr int DEC_PIECE = 8;                         // 64-bit mask words a thread of dec_occ_kernel counts: 512 cells
constexpr double DEC_ONE = 1048576.0;                // 2^20: the fixed point of the offsets
enum { DEC_BOX = 0, DEC_INVALID = 6, DEC_ERROR = 8, DEC_EMPTY = 9, DEC_OCCUPIED = 10,
       DEC_PARAMS = 12 /* doubles: lo.xyz, inv, n - 1 */, DEC_MISC_WORDS = 24 };

struct DecWs {
    uint32_t* misc;                                  // [DEC_MISC_WORDS]
    uint32_t* ref;                                   // [V] 1: a valid face names the vertex
    uint32_t* used;                                  // [K] by rank: a kept face names the cluster
    uint64_t* mask;                                  // [pieces * DEC_PIECE] bit c of the mask: cell c is occupied
    uint32_t* vrank;                                 // [V] referenced vertices: the cell, then (dec_rank_kernel) its rank
    uint32_t *fslot, *foff;                          // [F] the face's slot in `table` (DEC_NONE: invalid or degenerate); kept faces before it in its block
    uint32_t* table;                                 // [slots] face indices, DEC_NONE = empty
    uint32_t *spre, *oblk;                           // [pieces] occupied cells before the piece in its block; [oblocks] block totals, then scanned
    uint32_t *cellof, *uoff;                         // [K] by rank: the cell; used clusters before it in its block
    uint32_t *fblk, *ublk;                           // [fblocks], [kblocks] totals, then scanned
    uint32_t* lblk;                                  // [fblocks] faces with a slot (valid, not degenerate) in the block
    uint32_t* cnt;                                   // [K] by rank, emit: vertices of the cluster
    unsigned long long* sum;                         // [K, 3] by rank, emit: the sums of their offsets
    int64_t K, pieces, slots, oblocks, fblocks, kblocks, vblocks, zero_bytes, acc_bytes, bytes;
    __host__ DecWs(void* base, int64_t V, int64_t F, int64_t n) {
        MeshCarver c(base);                                              // base == nullptr: only the sizes are used
        const int64_t cells = n * n * n;
        K = V < cells ? V : cells;
        pieces = (cells + 64 * DEC_PIECE - 1) / (64 * DEC_PIECE);
        slots = 64;
        while (slots < 2 * F) slots *= 2;
        vblocks = (V + DEC_WG - 1) / DEC_WG;
        fblocks = (F + DEC_WG - 1) / DEC_WG;
        kblocks = (K + DEC_WG - 1) / DEC_WG;
        oblocks = (pieces + DEC_WG - 1) / DEC_WG;
        misc = c.take<uint32_t>(DEC_MISC_WORDS);                         // misc, ref, used, mask: zeroed by one memset of the count call
        ref = c.take<uint32_t>(V);
        used = c.take<uint32_t>(K);
        mask = c.take<uint64_t>(DEC_PIECE * pieces);
        zero_bytes = c.used();
        vrank = c.take<uint32_t>(V);
        fslot = c.take<uint32_t>(F);
        foff = c.take<uint32_t>(F);
        table = c.take<uint32_t>(slots);
        spre = c.take<uint32_t>(pieces);
        oblk = c.take<uint32_t>(oblocks);
        cellof = c.take<uint32_t>(K);
        uoff = c.take<uint32_t>(K);
        fblk = c.take<uint32_t>(fblocks);
        ublk = c.take<uint32_t>(kblocks);
        lblk = c.take<uint32_t>(fblocks);
        const int64_t acc = c.used();                                    // cnt, sum: zeroed by the memset of the emit call
        cnt = c.take<uint32_t>(K);
        sum = c.take<unsigned long long>(3 * K);
        acc_bytes = c.used() - acc;
        bytes = c.used();
    }
};

__device__ __forceinline__ const double* dec_params(const DecWs& ws) { return reinterpret_cast<const double*>(ws.misc + DEC_PARAMS); }

// The header's cell and fixed-point offset of a position, axis by axis; c in [0, n - 1] and q in [0, 2^20] whatever the input.
struct DecPlace {
    int c[3];
    uint32_t q[3];
};
__device__ __forceinline__ DecPlace dec_locate(const float* p, const double* params, int n) {
    DecPlace r;
    const double inv = params[3], last = params[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double u = ((double)p[k] - params[k]) * inv;
        const double fl = floor(u);
        r.c[k] = !(fl >= 0.0) ? 0 : (fl >= last ? n - 1 : (int)fl);      // a NaN lands in cell 0
        const double t = (u - (double)r.c[k]) * DEC_ONE;
        r.q[k] = !(t >= 0.0) ? 0u : (t >= DEC_ONE ? (uint32_t)DEC_ONE : (uint32_t)llrint(t));
    }
    return r;
}

__global__ __launch_bounds__(DEC_WG) void dec_ref_kernel(DgsMeshDecimateArgs a, DecWs ws) {
    const uint32_t f = blockIdx.x * DEC_WG + threadIdx.x, V = (uint32_t)a.V;
    const int lane = threadIdx.x & (DGS_WAVE - 1);
    bool invalid = false;
    if (f < (uint32_t)a.F) {
        const int32_t* t = a.faces + 3 * (size_t)f;
        const int i = t[0], j = t[1], k = t[2];
        if (mesh_face_valid(i, j, k, V)) {
            ws.ref[i] = 1;                                                // the same value from every writer
            ws.ref[j] = 1;
            ws.ref[k] = 1;
        } else {
            invalid = true;
        }
    }
    const uint64_t m = wave_ballot(invalid);
    if (m != 0 && lane == 0) atomicAdd(ws.misc + DEC_INVALID, (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(DEC_WG) void dec_box_kernel(DgsMeshDecimateArgs a, DecWs ws) {
    __shared__ uint32_t part[DEC_WG / DGS_WAVE][6];
    const uint32_t v = blockIdx.x * DEC_WG + threadIdx.x;
    const int lane = threadIdx.x & (DGS_WAVE - 1), wave = threadIdx.x >> 6;
    uint32_t key[6] = {0, 0, 0, 0, 0, 0};                                // 0: the identity of the maximum
    if (v < (uint32_t)a.V && ws.ref[v] != 0) {
        const float* p = a.vertices + 3 * (size_t)v;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t k = mesh_float_key(p[c]);
            key[c] = ~k;
            key[3 + c] = k;
        }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const uint32_t m = mesh_wave_max(key[c]);
        if (lane == 0) part[wave][c] = m;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        uint32_t m = 0;
#pragma unroll
        for (int w = 0; w < DEC_WG / DGS_WAVE; ++w) m = part[w][threadIdx.x] > m ? part[w][threadIdx.x] : m;
        if (m != 0) mesh_raise(ws.misc + DEC_BOX + threadIdx.x, m);
    }
}

// lo as doubles, inv = n / ext, n - 1, the EMPTY flag.  One wave; lane c < 3 converts the box of axis c, loaded per lane.
__global__ __launch_bounds__(DGS_WAVE) void dec_params_kernel(DgsMeshDecimateArgs a, DecWs ws, double nd) {
    __shared__ double extent[3];
    double* params = reinterpret_cast<double*>(ws.misc + DEC_PARAMS);
    if (threadIdx.x < 3) {
        const double lo = (double)mesh_float_unkey(~ws.misc[DEC_BOX + threadIdx.x]);
        extent[threadIdx.x] = (double)mesh_float_unkey(ws.misc[DEC_BOX + 3 + threadIdx.x]) - lo;
        params[threadIdx.x] = lo;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ext = extent[0];
        if (extent[1] > ext) ext = extent[1];
        if (extent[2] > ext) ext = extent[2];
        const bool empty = ws.misc[DEC_INVALID] >= (uint32_t)a.F || !(ext > 0.0);
        ws.misc[DEC_EMPTY] = empty ? 1u : 0u;
        params[3] = empty ? 0.0 : nd / ext;
        params[4] = nd - 1.0;
    }
}

__global__ __launch_bounds__(DEC_WG) void dec_cell_kernel(DgsMeshDecimateArgs a, DecWs ws) {
    if (ws.misc[DEC_EMPTY]) return;
    const uint32_t v = blockIdx.x * DEC_WG + threadIdx.x;
    if (v >= (uint32_t)a.V || ws.ref[v] == 0) return;
    const DecPlace at = dec_locate(a.vertices + 3 * (size_t)v, dec_params(ws), a.n);
    const uint32_t cell = ((uint32_t)at.c[0] * (uint32_t)a.n + (uint32_t)at.c[1]) * (uint32_t)a.n + (uint32_t)at.c[2];   // < n^3 <= 2^30
    ws.vrank[v] = cell;
    unsigned long long* word = reinterpret_cast<unsigned long long*>(ws.mask) + (cell >> 6);
    const unsigned long long bit = 1ull << (cell & 63);
    if (!(mesh_load(word) & bit)) atomicOr(word, bit);
}

__global__ __launch_bounds__(DEC_WG) void dec_occ_kernel(DecWs ws) {
    __shared__ uint32_t scratch[DEC_WG / DGS_WAVE + 1];
    if (ws.misc[DEC_EMPTY]) return;                                       // the whole grid
    const int64_t piece = (int64_t)blockIdx.x * DEC_WG + threadIdx.x;
    uint32_t here = 0;
    if (piece < ws.pieces) {
        const uint4* w = reinterpret_cast<const uint4*>(ws.mask + DEC_PIECE * piece);
#pragma unroll
        for (int j = 0; j < DEC_PIECE / 2; ++j) {
            const uint4 x = w[j];
            here += __popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w);
        }
    }
    uint32_t total;
    const uint32_t before = block_exclusive_scan<DEC_WG>(here, scratch, &total);
    if (piece < ws.pieces) ws.spre[piece] = before;
    if (threadIdx.x == 0) ws.oblk[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void dec_occ_sums_kernel(DecWs ws) {
    __shared__ uint32_t scratch[1024 / DGS_WAVE + 1];
    if (ws.misc[DEC_EMPTY]) return;
    const uint32_t occupied = mesh_scan_blocks(ws.oblk, ws.oblocks, scratch);
    if (threadIdx.x == 0) ws.misc[DEC_OCCUPIED] = occupied;
}

__global__ __launch_bounds__(DEC_WG) void dec_rank_kernel(DgsMeshDecimateArgs a, DecWs ws) {
    if (ws.misc[DEC_EMPTY]) return;
    const uint32_t v = blockIdx.x * DEC_WG + threadIdx.x;
    if (v >= (uint32_t)a.V || ws.ref[v] == 0) return;
    const uint32_t cell = ws.vrank[v], word = cell >> 6, piece = word / DEC_PIECE;
    uint32_t r = ws.oblk[piece / DEC_WG] + ws.spre[piece];
    for (uint32_t j = piece * DEC_PIECE; j < word; ++j) r += __popcll(ws.mask[j]);
    r += __popcll(ws.mask[word] & ((1ull << (cell & 63)) - 1));
    if (r >= (uint32_t)ws.K) {                                            // cannot be: occupied cells <= min(V, n^3).  Stay in range and say so
        ws.misc[DEC_ERROR] = 1;
        r = 0;
    }
    ws.vrank[v] = r;
    ws.cellof[r] = cell;                                                  // the same value from every writer
}

__global__ __launch_bounds__(DEC_WG) void dec_insert_kernel(DgsMeshDecimateArgs a, DecWs ws) {
    if (ws.misc[DEC_EMPTY]) return;
    const uint32_t f = blockIdx.x * DEC_WG + threadIdx.x, V = (uint32_t)a.V, slot_mask = (uint32_t)(ws.slots - 1);
    if (f < (uint32_t)a.F) {
        const int32_t* t = a.faces + 3 * (size_t)f;
        const int i = t[0], j = t[1], k = t[2];
        uint32_t mine = DEC_NONE;
        if (mesh_face_valid(i, j, k, V)) {
            const uint32_t ri = ws.vrank[i], rj = ws.vrank[j], rk = ws.vrank[k];
            if (ri != rj && ri != rk && rj != rk) {                           // otherwise degenerate: no slot
                const MeshTriple key = mesh_sorted(ri, rj, rk);
                uint32_t h = (key.s0 * 0x9E3779B1u) ^ (key.s1 * 0x85EBCA77u) ^ (key.s2 * 0xC2B2AE3Du);
                h ^= h >> 15;
                h *= 0x2C1B3C6Du;
                h ^= h >> 12;
                for (int64_t probe = 0; probe < ws.slots; ++probe) {
                    const uint32_t slot = (h + (uint32_t)probe) & slot_mask;
                    const uint32_t old = atomicCAS(ws.table + slot, DEC_NONE, f);
                    if (old == DEC_NONE) {
                        mine = slot;
                        break;
                    }
                    const int32_t* o = a.faces + 3 * (size_t)old;         // a face that was inserted: valid, not degenerate
                    const MeshTriple theirs = mesh_sorted(ws.vrank[o[0]], ws.vrank[o[1]], ws.vrank[o[2]]);
                    if (theirs.s0 == key.s0 && theirs.s1 == key.s1 && theirs.s2 == key.s2) {
                        if (f < old) atomicMin(ws.table + slot, f);
                        mine = slot;
                        break;
                    }
                }
                if (mine == DEC_NONE) ws.misc[DEC_ERROR] = 1;
            }
        }
        ws.fslot[f] = mine;
    }
}

__device__ __forceinline__ bool dec_face_kept(const DecWs& ws, uint32_t f, bool* live = nullptr) {
    const uint32_t slot = ws.fslot[f];
    if (live) *live = slot != DEC_NONE;
    return slot != DEC_NONE && ws.table[slot] == f;
}

__global__ __launch_bounds__(DEC_WG) void dec_fscan_kernel(DgsMeshDecimateArgs a, DecWs ws) {
    __shared__ uint32_t scratch[DEC_WG / DGS_WAVE + 1];
    if (ws.misc[DEC_EMPTY]) return;
    const uint32_t f = blockIdx.x * DEC_WG + threadIdx.x;
    bool live = false;
    const bool kept = f < (uint32_t)a.F && dec_face_kept(ws, f, &live);
    uint32_t total;                                                       // kept faces in the low half, faces with a slot in the high half: <= 256 each
    const uint32_t before = block_exclusive_scan<DEC_WG>((kept ? 1u : 0u) | (live ? 0x10000u : 0u), scratch, &total);
    if (f < (uint32_t)a.F) ws.foff[f] = before & 0xffffu;
    if (threadIdx.x == 0) {
        ws.fblk[blockIdx.x] = total & 0xffffu;
        ws.lblk[blockIdx.x] = total >> 16;
    }
    if (kept) {
        const int32_t* t = a.faces + 3 * (size_t)f;
#pragma unroll
        for (int c = 0; c < 3; ++c) ws.used[ws.vrank[t[c]]] = 1;          // the same value from every writer
    }
}

__global__ __launch_bounds__(DEC_WG) void dec_uscan_kernel(DecWs ws) {
    __shared__ uint32_t scratch[DEC_WG / DGS_WAVE + 1];
    if (ws.misc[DEC_EMPTY]) return;
    const int64_t r = (int64_t)blockIdx.x * DEC_WG + threadIdx.x;
    uint32_t total;
    const uint32_t before = block_exclusive_scan<DEC_WG>(r < ws.K && ws.used[r] != 0 ? 1u : 0u, scratch, &total);
    if (r < ws.K) ws.uoff[r] = before;
    if (threadIdx.x == 0) ws.ublk[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void dec_sums_kernel(DgsMeshDecimateArgs a, DecWs ws) {
    __shared__ uint32_t scratch[1024 / DGS_WAVE + 1];
    const uint32_t F = (uint32_t)a.F, invalid = ws.misc[DEC_INVALID];
    if (ws.misc[DEC_ERROR]) {
        if (threadIdx.x < 5) a.counts[threadIdx.x] = DEC_NONE;
        return;
    }
    if (ws.misc[DEC_EMPTY]) {                                             // every valid face counts as degenerate
        if (threadIdx.x < 5) a.counts[threadIdx.x] = threadIdx.x == 2 ? F - invalid : threadIdx.x == 4 ? invalid : 0u;
        return;
    }
    const uint32_t nv = mesh_scan_blocks(ws.ublk, ws.kblocks, scratch);
    const uint32_t nf = mesh_scan_blocks(ws.fblk, ws.fblocks, scratch);
    const uint32_t live = mesh_scan_blocks(ws.lblk, ws.fblocks, scratch);
    if (threadIdx.x == 0) {
        const uint32_t degenerate = F - invalid - live;
        a.counts[0] = nv;
        a.counts[1] = nf;
        a.counts[2] = degenerate;
        a.counts[3] = F - invalid - degenerate - nf;
        a.counts[4] = invalid;
    }
}

// V = 0 or F = 0: nothing is output; with no vertices every face is invalid.
__global__ void dec_nothing_kernel(uint32_t* counts, uint32_t invalid) {
    if (threadIdx.x < 5) counts[threadIdx.x] = threadIdx.x == 4 ? invalid : 0u;
}

__global__ __launch_bounds__(DEC_WG) void dec_accumulate_kernel(DgsMeshDecimateArgs a, DecWs ws) {
    if (ws.misc[DEC_EMPTY] || ws.misc[DEC_ERROR]) return;
    const uint32_t v = blockIdx.x * DEC_WG + threadIdx.x;
    if (v >= (uint32_t)a.V || ws.ref[v] == 0) return;
    const uint32_t r = ws.vrank[v];
    if (ws.used[r] == 0) return;
    const DecPlace at = dec_locate(a.vertices + 3 * (size_t)v, dec_params(ws), a.n);
    atomicAdd(ws.cnt + r, 1u);
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(ws.sum + 3 * (size_t)r + k, (unsigned long long)at.q[k]);
}

__global__ __launch_bounds__(DEC_WG) void dec_emit_vertices_kernel(DgsMeshDecimateArgs a, DecWs ws) {
    if (ws.misc[DEC_EMPTY] || ws.misc[DEC_ERROR]) return;
    const int64_t r = (int64_t)blockIdx.x * DEC_WG + threadIdx.x;
    if (r >= ws.K || ws.used[r] == 0) return;
    const uint32_t at = ws.ublk[blockIdx.x] + ws.uoff[r];
    if ((int64_t)at >= a.max_vertices) return;
    const double* params = dec_params(ws);
    const uint32_t n = (uint32_t)a.n, cell = ws.cellof[r];
    const uint32_t c[3] = {cell / (n * n), cell / n % n, cell % n};
    const double weight = (double)ws.cnt[r] * DEC_ONE, inv = params[3];
    float* out = a.out_vertices + 3 * (size_t)at;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double mean = (double)ws.sum[3 * (size_t)r + k] / weight;   // each operation rounded on its own: STRICT_FP
        const double inside = (double)c[k] + mean;
        out[k] = (float)(params[k] + inside / inv);
    }
}

__global__ __launch_bounds__(DEC_WG) void dec_emit_faces_kernel(DgsMeshDecimateArgs a, DecWs ws) {
    if (ws.misc[DEC_EMPTY] || ws.misc[DEC_ERROR]) return;
    const uint32_t f = blockIdx.x * DEC_WG + threadIdx.x;
    if (f >= (uint32_t)a.F || !dec_face_kept(ws, f)) return;
    const uint32_t at = ws.fblk[blockIdx.x] + ws.foff[f];
    if ((int64_t)at >= a.max_faces) return;
    const int32_t* t = a.faces + 3 * (size_t)f;
    int32_t* out = a.out_faces + 3 * (size_t)at;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t r = ws.vrank[t[c]];
        out[c] = (int32_t)(ws.ublk[r / DEC_WG] + ws.uoff[r]);
    }
}

static bool dec_args_ok(const DgsMeshDecimateArgs* a) {
    return a && a->V >= 0 && a->F >= 0 && a->V <= DEC_MAX_ROWS && a->F <= DEC_MAX_ROWS && a->n >= 1 && a->n <= DEC_MAX_N &&
           (a->V == 0 || a->vertices) && (a->F == 0 || a->faces) && a->workspace && ((uintptr_t)a->workspace & 15) == 0 &&
           a->workspace_bytes >= DecWs(nullptr, a->V, a->F, a->n).bytes;
}

}  // namespace dgs

extern "C" int64_t dgs_mesh_decimate_workspace_bytes(int64_t V, int64_t F, int32_t n) {
    if (V < 0 || F < 0 || V > dgs::DEC_MAX_ROWS || F > dgs::DEC_MAX_ROWS || n < 1 || n > dgs::DEC_MAX_N) return 0;
    return dgs::DecWs(nullptr, V, F, n).bytes;
}

extern "C" int dgs_mesh_decimate_count(const DgsMeshDecimateArgs* a, dgs_stream_t stream) {
    using namespace dgs;
    if (!dec_args_ok(a) || !a->counts) return DGS_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a->V == 0 || a->F == 0) {
        hipLaunchKernelGGL(dec_nothing_kernel, dim3(1), dim3(DGS_WAVE), 0, st, a->counts, (uint32_t)(a->V == 0 ? a->F : 0));
        return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
    }
    const DecWs ws(a->workspace, a->V, a->F, a->n);
    const dim3 wg(DEC_WG), vgrid((unsigned)ws.vblocks), fgrid((unsigned)ws.fblocks);
    if (hipMemsetAsync(ws.misc, 0, (size_t)ws.zero_bytes, st) != hipSuccess) return DGS_ERR_DEVICE;
    if (hipMemsetAsync(ws.table, 0xff, 4 * (size_t)ws.slots, st) != hipSuccess) return DGS_ERR_DEVICE;
    hipLaunchKernelGGL(dec_ref_kernel, fgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(dec_box_kernel, vgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(dec_params_kernel, dim3(1), dim3(DGS_WAVE), 0, st, *a, ws, (double)a->n);
    hipLaunchKernelGGL(dec_cell_kernel, vgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(dec_occ_kernel, dim3((unsigned)ws.oblocks), wg, 0, st, ws);
    hipLaunchKernelGGL(dec_occ_sums_kernel, dim3(1), dim3(1024), 0, st, ws);
    hipLaunchKernelGGL(dec_rank_kernel, vgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(dec_insert_kernel, fgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(dec_fscan_kernel, fgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(dec_uscan_kernel, dim3((unsigned)ws.kblocks), wg, 0, st, ws);
    hipLaunchKernelGGL(dec_sums_kernel, dim3(1), dim3(1024), 0, st, *a, ws);
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}

extern "C" int dgs_mesh_decimate_emit(const DgsMeshDecimateArgs* a, dgs_stream_t stream) {
    using namespace dgs;
    if (!dec_args_ok(a) || a->max_vertices < 0 || a->max_faces < 0 || (a->max_vertices > 0 && !a->out_vertices) || (a->max_faces > 0 && !a->out_faces))
        return DGS_ERR_INVALID_ARGUMENT;
    if (a->V == 0 || a->F == 0) return DGS_OK;                            // nothing is output
    hipStream_t st = static_cast<hipStream_t>(stream);
    const DecWs ws(a->workspace, a->V, a->F, a->n);
    if (a->max_vertices > 0) {
        if (hipMemsetAsync(ws.cnt, 0, (size_t)ws.acc_bytes, st) != hipSuccess) return DGS_ERR_DEVICE;
        hipLaunchKernelGGL(dec_accumulate_kernel, dim3((unsigned)ws.vblocks), dim3(DEC_WG), 0, st, *a, ws);
        hipLaunchKernelGGL(dec_emit_vertices_kernel, dim3((unsigned)ws.kblocks), dim3(DEC_WG), 0, st, *a, ws);
    }
    if (a->max_faces > 0) hipLaunchKernelGGL(dec_emit_faces_kernel, dim3((unsigned)ws.fblocks), dim3(DEC_WG), 0, st, *a, ws);
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}
