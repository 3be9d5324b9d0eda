// mesh_common.h -- what the mesh stages after marching cubes share: mesh_clean.hip, mesh_decimate.hip, mesh_smooth.hip, mesh_repair.hip
// (and mesh.hip for the workspace carver).  Every function is __forceinline__, so each file has its own copy of the instructions and
// nothing meets at link time.
//   mesh_face_valid                       three indices inside [0, V)
//   mesh_load, mesh_raise                 the agent-scope atomic load, and the atomicMax that looks first
//   mesh_float_key / mesh_float_unkey     the order-preserving uint32 image of a float
//   mesh_wave_max                         the maximum over a wave
//   mesh_find / mesh_union                the lock-free union-find
//   mesh_scan_blocks                      one workgroup of 1,024 scans a list of block totals
//   MeshTriple, mesh_sorted               the key of the open-addressing tables of faces
//   mesh_copy_vertex_bytes                a vertex as its 12 bytes
//   MeshCarver                            (host) the pieces of a workspace, each rounded up to 16 bytes
#ifndef DGS_MESH_COMMON_H
#define DGS_MESH_COMMON_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "dgs_device.h"

namespace dgs {

// The pieces of a workspace one after another from `base`, each rounded up to 16 bytes.  base == nullptr: only the sizes are used.
struct MeshCarver {
    uintptr_t base, at;
    explicit MeshCarver(void* p) : base(reinterpret_cast<uintptr_t>(p)), at(base) {}
    template <class T>
    T* take(int64_t count) {
        const uintptr_t p = at;
        at += (uintptr_t)(((int64_t)sizeof(T) * count + 15) & ~(int64_t)15);
        return reinterpret_cast<T*>(p);
    }
    int64_t used() const { return (int64_t)(at - base); }
};

__device__ __forceinline__ bool mesh_face_valid(int a, int b, int c, uint32_t V) { return (uint32_t)a < V && (uint32_t)b < V && (uint32_t)c < V; }

// A relaxed agent-scope atomic load (32 or 64 bits): the value in memory, not a line this XCD's L2 may still hold from before another
// XCD's atomic.  The XCDs' L2s are not coherent for plain loads inside a launch, so a word that atomics of the same launch write is
// read with this and nothing else.
template <class T>
__device__ __forceinline__ T mesh_load(T* p) {
#ifdef HIPEMU
    return *p;
#else
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

// atomicMax that first looks: the words only grow, so a value that does not exceed what is there already needs no atomic.  Nearly
// every wave inside a large component is in that position, and the atomics of one address are served one after another.
__device__ __forceinline__ void mesh_raise(uint32_t* p, uint32_t v) {
    if (v > mesh_load(p)) atomicMax(p, v);
}

// Order-preserving image of a float: a < b as floats <=> key(a) < key(b) as unsigned (-0 below +0; a NaN is just some key).  A minimum
// is kept as the maximum of the complemented keys, so that zero is the identity of minima and maxima alike.
__device__ __forceinline__ uint32_t mesh_float_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float mesh_float_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? k & 0x7fffffffu : ~k); }

__device__ __forceinline__ uint32_t mesh_wave_max(uint32_t v) {
#pragma unroll
    for (int d = 1; d < DGS_WAVE; d <<= 1) {
        const uint32_t o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

// ---- lock-free union-find over indices below 2^32, started from parent[x] = x (or from any forest with parent[x] <= x) ----
// A root is hooked under a SMALLER root with one atomicCAS on its own parent word, and path halving only ever lowers a parent (atomicMin
// to a grandparent), so parent[x] <= x always holds, no cycle can form and the root of a tree is the smallest index of its set.  Nothing
// waits: a CAS that loses starts over from the new roots.  EVERY access to parent[] in the launch that unites is an agent-scope atomic
// (mesh_load, atomicMin, atomicCAS); the next launch reads the final links with plain loads.
// Root of x, halving the path: parent[x] is lowered to x's grandparent, an ancestor with a smaller index.
__device__ __forceinline__ uint32_t mesh_find(uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = mesh_load(parent + x);
        if (p == x) return x;
        const uint32_t g = mesh_load(parent + p);
        if (g == p) return p;
        atomicMin(parent + x, g);
        x = g;
    }
}

// -> the root of the united set at the time of the call.
__device__ __forceinline__ uint32_t mesh_union(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = mesh_find(parent, a);
        b = mesh_find(parent, b);
        if (a == b) return a;
        const uint32_t big = a > b ? a : b, small = a > b ? b : a;
        if (atomicCAS(parent + big, big, small) == big) return small;   // `big` was still a root: hooked.  Otherwise someone hooked it first: again
    }
}

// Exclusive scan of n block totals in place by one workgroup of 1,024: a contiguous piece a thread, as long as it has to be, and a scan
// of the pieces' sums -> the sum of all.  `scratch` as block_exclusive_scan<1024> takes it.
__device__ __forceinline__ uint32_t mesh_scan_blocks(uint32_t* blk, int64_t n, uint32_t* scratch) {
    const int64_t per = (n + 1023) / 1024, c0 = per * threadIdx.x, c1 = c0 + per < n ? c0 + per : n;
    uint32_t s = 0;
    for (int64_t c = c0; c < c1; ++c) s += blk[c];
    uint32_t total;
    uint32_t run = block_exclusive_scan<1024>(s, scratch, &total);
    for (int64_t c = c0; c < c1; ++c) {
        const uint32_t here = blk[c];
        blk[c] = run;
        run += here;
    }
    return total;
}

// Three indices in ascending order: the key of a face in an open-addressing table, whichever corner comes first.  The four lines
// that hash it stay written out in dec_insert_kernel and rep_dup_slot: behind a function of its own hipcc combines the three products
// in another order, and the kernels' instructions would no longer be the ones that were measured.
struct MeshTriple {
    uint32_t s0, s1, s2;                                                  // ascending
};
__device__ __forceinline__ MeshTriple mesh_sorted(uint32_t x, uint32_t y, uint32_t z) {
    uint32_t t;
    if (x > y) { t = x; x = y; y = t; }
    if (y > z) { t = y; y = z; z = t; }
    if (x > y) { t = x; x = y; y = t; }
    return {x, y, z};
}

// Row v of `in` to row `at` of `out` as 12 bytes, not three floats: NaN payloads stay.
__device__ __forceinline__ void mesh_copy_vertex_bytes(const float* in, uint32_t v, float* out, uint32_t at) {
    const uint32_t* from = reinterpret_cast<const uint32_t*>(in) + 3 * (size_t)v;
    uint32_t* to = reinterpret_cast<uint32_t*>(out) + 3 * (size_t)at;
    to[0] = from[0];
    to[1] = from[1];
    to[2] = from[2];
}

}  // namespace dgs

#endif  // DGS_MESH_COMMON_H
