/* dgs_ema.h -- C ABI of the exponential moving average of the weights (the reference trains with `EMA(decay=0.9999)` and
 * `EMAModelCheckpoint` unless --use_ema is off, launch.py:205-228; validation and test run on the averaged weights,
 * diffusionGS/utils/ema.py:167-181).
 *
 * The shadows are kept by the launch that updates the parameters (dgs_adamw_ema_step: include/dgs_optim.h's step with 8 more bytes
 * per parameter), and evaluation on the averaged weights rewrites only the engine's bf16 / fp32 / transposed operand copies
 * (dgs_ema_apply): the fp32 master parameters never move.
 *
 * Arithmetic = the reference's non-apex form (utils/ema.py:94-101), on the NEW parameter value, three separately rounded fp32
 * operations (never contracted into an FMA), bit for bit what torch computes:
 *     d = ema - p;  d = d * one_minus_decay;  ema = ema - d
 * one_minus_decay is computed by the caller as (float)(1.0 - (double)decay): the scalar torch's `mul_(1.0 - decay)` multiplies an
 * fp32 tensor by.  Device pointers, a HIP stream, no host synchronisation; returns DGS_OK or a negative DgsStatus.
 */
#ifndef DGS_EMA_H
#define DGS_EMA_H

#include <stdint.h>

#include "dgs_optim.h" /* DgsAdamWArgs, DGS_OPTIM_COPY_*, DgsStatus, dgs_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- fused into the AdamW launch -------------------------------------------------------------------------------------------------
 * The shadows live in ONE flat fp32 buffer laid out exactly like the buffer the first moments live in (DgsAdamWTensor.m of every
 * entry = m_base + its offset): the kernel finds a tensor's shadow at ema_base + (t.m - m_base), and the planned table is the one
 * dgs_adamw_step takes.  Both bases 16-byte aligned. */
typedef struct DgsEmaFusedArgs {
    float* ema_base;
    const float* m_base;
    float one_minus_decay;
} DgsEmaFusedArgs;

/* dgs_adamw_step + the EMA update of every tensor of the table, one launch.  A non-finite gradient norm skips the shadows with the
 * update. */
int dgs_adamw_ema_step(const DgsAdamWArgs* args, const DgsEmaFusedArgs* ema, dgs_stream_t stream);

/* ---- table-driven launch for everything else -------------------------------------------------------------------------------------
 * One tensor: `rows` x `cols` row-major (a vector: rows = 1).  A tensor with a transposed copy needs rows % 64 == 0 and
 * cols % 64 == 0; `first_tile` is filled in by dgs_ema_plan.  Tiling as in dgs_adamw_step: 4,096-element flat tiles, 64 x 64 blocks
 * through LDS for a transposed bf16 copy. */
typedef struct DgsEmaTensor {
    const float* p;    /* fp32 master parameter: read, never written                                 */
    float* ema;        /* its shadow                                                                */
    void* copy;        /* optional row-major copy [rows, cols]: bf16 or f32                          */
    void* copy_t;      /* optional transposed bf16 copy [cols, rows]                                */
    int64_t rows, cols;
    int32_t copy_kind; /* DGS_OPTIM_COPY_*                                                          */
    int32_t first_tile;
} DgsEmaTensor;

#define DGS_EMA_SOURCE_NONE 0 /* the copies are not written                                          */
#define DGS_EMA_SOURCE_P 1    /* copies = the parameters (swap out: back to the raw weights)         */
#define DGS_EMA_SOURCE_EMA 2  /* copies = the shadows (swap in: evaluate on the averaged weights)    */

typedef struct DgsEmaArgs {
    const DgsEmaTensor* tensors; /* DEVICE pointer to the planned table                              */
    int32_t n_tensors;
    int32_t n_tiles;             /* value returned by dgs_ema_plan                                   */
    float one_minus_decay;       /* read when update != 0                                           */
    int32_t update;              /* != 0: ema = ema - (ema - p) * one_minus_decay first               */
    int32_t copy_source;         /* DGS_EMA_SOURCE_*; with update != 0, DGS_EMA_SOURCE_EMA copies the NEW shadow */
} DgsEmaArgs;

/* HOST: fills `first_tile` of every entry of a host-side table and returns the launch's tile count (< 0: invalid table; the alignment
 * rules are dgs_adamw_plan's: p / ema 16 bytes, a bf16 copy 8, any other copy 16).  Copy the table to the device afterwards. */
int32_t dgs_ema_plan(DgsEmaTensor* host_tensors, int32_t n_tensors);

/* One launch over the table: the EMA update (update != 0) and / or the copies written from `copy_source`.  Neither: invalid. */
int dgs_ema_apply(const DgsEmaArgs* args, dgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
