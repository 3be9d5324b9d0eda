// lpips_mfma.h -- the f32-input MFMA of csrc/lpips.hip: v_mfma_f32_32x32x2_f32 on the device, and its restatement for the CPU
// emulation build (tests/hipemu emulates the bf16 / f16 forms only).
//
// Operands (cdna_hip_programming.md section 3): lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31], one f32 each;
// C / D: register r of lane l is D[row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col = l & 31].  The result is the k-ordered chain
// D = fma(A[i][1], B[1][j], fma(A[i][0], B[0][j], C)): one rounding per product, nothing wider inside.
#pragma once
#include <hip/hip_runtime.h>

namespace dgs {

typedef float lpips_f32x16 __attribute__((ext_vector_type(16)));

#ifdef HIPEMU
inline lpips_f32x16 mfma_f32_32x32x2(float a, float b, lpips_f32x16 c) {
    struct P { float a, b; } p{a, b};
    hipemu::Sync& s = hipemu::my_wave();
    const int me = hipemu::ctx().cur->lane;
    const int buf = hipemu::arrive(s, me, &p, sizeof(P));
    const int col = me & 31;
    lpips_f32x16 d = c;
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (me >> 5);
        float acc = c[r];
        for (int k = 0; k < 2; ++k)
            acc = fmaf(hipemu::snap_get<P>(s, buf, row + 32 * k).a, hipemu::snap_get<P>(s, buf, col + 32 * k).b, acc);
        d[r] = acc;
    }
    return d;
}
#else
__device__ __forceinline__ lpips_f32x16 mfma_f32_32x32x2(float a, float b, lpips_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
#endif

}  // namespace dgs
