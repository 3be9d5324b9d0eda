// store_tail_bench.hip -- what does the output of a one-round kernel cost when every workgroup stores it in its last microseconds,
// and does the store's cache policy change that?  The DiT step's B = 1 kernels are one-round grids: a workgroup computes for
// 25-90 us and then writes its whole tile through store_strip's row-major pass (16 bytes per lane, a wave-instruction = 1 KiB of
// whole 512-byte row segments at the tensor's row stride).  Here the compute is a timed idle on the constant 100 MHz clock
// (wall_clock64), followed by exactly that store pattern under one of three policies:
//     plain    global_store_dwordx4                 (write-back: the lines stay dirty in the XCD's L2 until the kernel ends)
//     nt       __builtin_nontemporal_store          (global_store_dwordx4 ... nt)
//     sc1      global_store_dwordx4 ... sc1         (agent scope, performed at the memory side: write-through; st_agent4 of
//                                                    csrc/dit_common.h)
// with or without ~40 VALU instructions per 16-byte store between the stores (stands in for fc1's GELU).  Every launch is followed
// by a DEPENDENT 256-workgroup kernel that reads 16 bytes per workgroup of what was just written, so the boundary behind the
// writer is a true dependency; what it read is checked on the host once per configuration.  Per configuration:
//     epi mean = mean over workgroups of (all stores performed - idle over)      the epilogue as one workgroup sees it
//     epi last = last workgroup's end - mean end of the idle                     the epilogue as the launch sees it
//     gap      = first start of the reader - last end of the writer              what the kernel end costs (write-back included)
//     pair     = HIP events around the whole sequence / pairs, minus the idle    everything beyond the idle per writer + reader
// and the pair once more with the same sequence captured in one hipGraph.  The only loop is the timed idle: nothing spins on memory.
//   hipcc --offload-arch=gfx950 -O2 -o store_tail_bench store_tail_bench.hip && ./store_tail_bench
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

enum Policy { PLAIN = 0, NT = 1, SC1 = 2 };
static const char* policy_name[3] = {"plain", "nt", "sc1"};

typedef float f32x4_t __attribute__((ext_vector_type(4)));

struct Payload {
    const char* name;
    int grid, threads;
    int wg_bytes;      // bytes one workgroup writes
    int seg_bytes;     // contiguous bytes of one tensor row inside the workgroup's tile
    int stride_bytes;  // the tensor's row stride
    int tiles_x;       // tiles side by side in a row of the tensor (tiles_x * seg_bytes <= stride_bytes)
    bool rmw;          // fp32 read (before the idle) - modify - write in place
};

// the value of 16-byte chunk `q` (global chunk index = byte offset / 16) of launch `launch`, before the filler
__host__ __device__ inline float seed_value(uint32_t q, int comp, int launch) {
    return (float)((q * 4u + (uint32_t)comp + 977u * (uint32_t)launch) & 0xffffu) * (1.0f / 65536.0f);
}
// ~40 VALU per 16-byte store: ten dependent fmas per component
__host__ __device__ inline float filler(float x) {
#pragma unroll
    for (int i = 0; i < 10; ++i) x = fmaf(x, 0.999f, 0.001f);
    return x;
}

template <int POLICY>
__device__ __forceinline__ void store16(float* ptr, f32x4_t v) {
    if (POLICY == PLAIN) *reinterpret_cast<f32x4_t*>(ptr) = v;
    else if (POLICY == NT) __builtin_nontemporal_store(v, reinterpret_cast<f32x4_t*>(ptr));
    else asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(ptr), "v"(v) : "memory");   // s_nop: the store-data hazard hipcc cannot see in asm
}

// byte offset of the workgroup's 16-byte chunk i (0 .. wg_bytes / 16)
__host__ __device__ inline size_t chunk_offset(const Payload& p, int wg, int i) {
    const int cpr = p.seg_bytes / 16, rows = p.wg_bytes / p.seg_bytes;
    const int tx = wg % p.tiles_x, ty = wg / p.tiles_x;
    return ((size_t)ty * rows + i / cpr) * p.stride_bytes + (size_t)tx * p.seg_bytes + (size_t)(i % cpr) * 16;
}

constexpr int MAX_IT = 16;     // 128 KiB per workgroup of 512 threads

template <int POLICY, bool FILL>
__global__ void writer_kernel(char* out, Payload p, long long spin_ticks, int launch, unsigned long long* stamps) {
    const int its = p.wg_bytes / (blockDim.x * 16);
    f32x4_t old[MAX_IT / 2];
    if (p.rmw) {
#pragma unroll
        for (int it = 0; it < MAX_IT / 2; ++it)
            if (it < its) old[it] = *reinterpret_cast<const f32x4_t*>(out + chunk_offset(p, blockIdx.x, it * blockDim.x + threadIdx.x));
    }
    const unsigned long long t0 = wall_clock64();
    while ((long long)(wall_clock64() - t0) < spin_ticks) __builtin_amdgcn_s_sleep(2);
    const unsigned long long t1 = wall_clock64();
    launch += t1 == 0 ? 1 : 0;                             // never: keeps the values' arithmetic behind the idle
#pragma unroll
    for (int it = 0; it < MAX_IT; ++it) {
        if (it < its) {
            const size_t o = chunk_offset(p, blockIdx.x, it * blockDim.x + threadIdx.x);
            const uint32_t q = (uint32_t)(o >> 4);
            f32x4_t v = {seed_value(q, 0, launch), seed_value(q, 1, launch), seed_value(q, 2, launch), seed_value(q, 3, launch)};
            if (FILL) v = f32x4_t{filler(v.x), filler(v.y), filler(v.z), filler(v.w)};
            if (p.rmw) { if (it < MAX_IT / 2) v += old[it]; }
            store16<POLICY>(reinterpret_cast<float*>(out + o), v);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every store of this wave performed (in L2 / at the memory side)
    __syncthreads();
    const unsigned long long t2 = wall_clock64();
    if (threadIdx.x == 0) {
        unsigned long long* s = stamps + ((size_t)launch * gridDim.x + blockIdx.x) * 3;
        s[0] = t0; s[1] = t1; s[2] = t2;
    }
}

// workgroup b reads the LAST 16-byte chunk of writer workgroup (b * step) % writers
__global__ void reader_kernel(const char* out, Payload p, int step, int launch, f32x4_t* seen, unsigned long long* stamps) {
    const unsigned long long t0 = wall_clock64();
    if (threadIdx.x == 0) {
        const int wg = (int)(((long long)blockIdx.x * step) % p.grid);
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(out + chunk_offset(p, wg, p.wg_bytes / 16 - 1));
        seen[(size_t)launch * gridDim.x + blockIdx.x] = v;
        unsigned long long* s = stamps + ((size_t)launch * gridDim.x + blockIdx.x) * 2;
        s[0] = t0; s[1] = wall_clock64();
    }
}

typedef void (*writer_fn)(char*, Payload, long long, int, unsigned long long*);
static writer_fn writers[3][2] = {{writer_kernel<PLAIN, false>, writer_kernel<PLAIN, true>},
                                  {writer_kernel<NT, false>, writer_kernel<NT, true>},
                                  {writer_kernel<SC1, false>, writer_kernel<SC1, true>}};

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

static const int READERS = 256;

struct Result { double epi_mean, epi_last, gap, pair_us; bool ok; };

static Result run(const Payload& p, int policy, bool fill, double spin_us, int N, bool graph) {
    const int rows = p.wg_bytes / p.seg_bytes, tiles_y = (p.grid + p.tiles_x - 1) / p.tiles_x;
    const size_t bytes = (size_t)tiles_y * rows * p.stride_bytes;
    // bounds, checked before anything runs: whole 16-byte chunks per thread, tiles inside the row, registers enough for the rmw form
    if (p.wg_bytes % (p.threads * 16) || p.wg_bytes / (p.threads * 16) > MAX_IT || p.wg_bytes % p.seg_bytes || p.seg_bytes % 16 ||
        (size_t)p.tiles_x * p.seg_bytes > (size_t)p.stride_bytes || (p.rmw && p.wg_bytes / (p.threads * 16) > MAX_IT / 2) ||
        chunk_offset(p, p.grid - 1, p.wg_bytes / 16 - 1) + 16 > bytes) {
        fprintf(stderr, "bad payload %s\n", p.name);
        exit(1);
    }
    char* out;
    unsigned long long *wst, *rst;
    f32x4_t* seen;
    CK(hipMalloc(&out, bytes));
    CK(hipMemset(out, 0, bytes));
    CK(hipMalloc(&wst, (size_t)N * p.grid * 24));
    CK(hipMalloc(&rst, (size_t)N * READERS * 16));
    CK(hipMalloc(&seen, (size_t)N * READERS * 16));
    const long long ticks = (long long)(spin_us * 100.0);
    const int step = 37;                                      // odd: readers visit writer tiles of every XCD
    hipStream_t st;
    hipEvent_t e0, e1;
    CK(hipStreamCreate(&st));
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    writer_fn w = writers[policy][fill ? 1 : 0];
    auto sequence = [&]() {
        for (int i = 0; i < N; ++i) {
            hipLaunchKernelGGL(w, dim3(p.grid), dim3(p.threads), 0, st, out, p, ticks, i, wst);
            hipLaunchKernelGGL(reader_kernel, dim3(READERS), dim3(64), 0, st, (const char*)out, p, step, i, seen, rst);
        }
    };
    hipGraphExec_t exec = nullptr;
    hipGraph_t g = nullptr;
    if (graph) {
        CK(hipStreamBeginCapture(st, hipStreamCaptureModeGlobal));
        sequence();
        CK(hipStreamEndCapture(st, &g));
        CK(hipGraphInstantiate(&exec, g, nullptr, nullptr, 0));
    }
    float ms = 0;
    for (int rep = 0; rep < 2; ++rep) {                       // the second pass is the measured one
        CK(hipMemsetAsync(out, 0, bytes, st));
        CK(hipStreamSynchronize(st));
        CK(hipEventRecord(e0, st));
        if (graph) CK(hipGraphLaunch(exec, st));
        else sequence();
        CK(hipEventRecord(e1, st));
        CK(hipStreamSynchronize(st));
    }
    CK(hipGetLastError());
    CK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<unsigned long long> hw((size_t)N * p.grid * 3), hr((size_t)N * READERS * 2);
    std::vector<f32x4_t> hs((size_t)N * READERS);
    CK(hipMemcpy(hw.data(), wst, hw.size() * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hr.data(), rst, hr.size() * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hs.data(), seen, hs.size() * 16, hipMemcpyDeviceToHost));
    Result r{0, 0, 0, ms * 1e3 / N - spin_us, true};
    for (int i = 0; i < N; ++i) {
        double se_mean = 0, epi = 0;
        unsigned long long e_max = 0, n_min = ~0ull;
        for (int b = 0; b < p.grid; ++b) {
            const unsigned long long* s = &hw[((size_t)i * p.grid + b) * 3];
            se_mean += (double)(s[1] - hw[(size_t)i * p.grid * 3]);
            epi += (double)(s[2] - s[1]);
            e_max = std::max(e_max, s[2]);
        }
        for (int b = 0; b < READERS; ++b) n_min = std::min(n_min, hr[((size_t)i * READERS + b) * 2]);
        r.epi_mean += epi / p.grid * 0.01;
        r.epi_last += ((double)(e_max - hw[(size_t)i * p.grid * 3]) - se_mean / p.grid) * 0.01;
        r.gap += ((double)n_min - (double)e_max) * 0.01;
    }
    r.epi_mean /= N; r.epi_last /= N; r.gap /= N;
    // what every reader saw after every launch
    for (int b = 0; b < READERS; ++b) {
        const uint32_t q = (uint32_t)(chunk_offset(p, (int)(((long long)b * step) % p.grid), p.wg_bytes / 16 - 1) >> 4);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < N; ++i)
            for (int c = 0; c < 4; ++c) {
                float v = seed_value(q, c, i);
                if (fill) v = filler(v);
                acc[c] = p.rmw ? acc[c] + v : v;
                if (hs[(size_t)i * READERS + b][c] != acc[c]) r.ok = false;
            }
    }
    if (graph) { CK(hipGraphExecDestroy(exec)); CK(hipGraphDestroy(g)); }
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1)); CK(hipStreamDestroy(st));
    CK(hipFree(out)); CK(hipFree(wst)); CK(hipFree(rst)); CK(hipFree(seen));
    return r;
}

int main(int argc, char** argv) {
    const int N = argc > 1 ? atoi(argv[1]) : 100;
    // name, grid, threads, bytes per workgroup, row segment, row stride, tiles per row, rmw
    const Payload payloads[] = {
        {"fc1  h bf16 128K", 256, 512, 131072, 512, 8192, 16, false},     // 4096 x 4096 bf16, 33.5 MB
        {"qkv  q|k bf16 64K", 256, 512, 65536, 512, 4096, 8, false},      // 4096 x 2048 bf16, 16.8 MB
        {"gate f32 rmw 64K", 256, 512, 65536, 512, 4096, 8, true},        // 4096 x 1024 fp32 in place, 16.8 MB
        {"attn ao bf16 32K", 256, 512, 32768, 512, 2048, 4, false},       // 4096 x 1024 bf16, 8.4 MB
        {"ln   xn bf16  8K", 1088, 256, 8192, 2048, 2048, 1, false},      // 4352 x 1024 bf16, four whole rows per workgroup
    };
    printf("%d writer + dependent reader pairs per configuration; times in us; pair = events per pair - idle\n", N);
    printf("%-18s %-5s %-4s %5s | %8s %8s %7s %8s | %8s | %s\n", "payload", "store", "fill", "idle", "epi mean", "epi last", "gap", "pair", "graph pr", "values");
    for (const Payload& p : payloads)
        for (double us : {25.0, 75.0})
            for (int fill = 0; fill < 2; ++fill)
                for (int pol = 0; pol < 3; ++pol) {
                    const Result s = run(p, pol, fill != 0, us, N, false), g = run(p, pol, fill != 0, us, N, true);
                    printf("%-18s %-5s %-4s %5.0f | %8.2f %8.2f %7.2f %8.2f | %8.2f | %s\n", p.name, policy_name[pol], fill ? "yes" : "no", us, s.epi_mean, s.epi_last,
                           s.gap, s.pair_us, g.pair_us, s.ok && g.ok ? "ok" : "MISMATCH");
                    fflush(stdout);
                }
    return 0;
}
