// ema_arith.h -- the one EMA expression, shared by the fused AdamW launch (optim.hip) and the table-driven launch (ema.hip).
#pragma once
#include "dgs_device.h"

namespace dgs {

// The reference's non-apex form (utils/ema.py:94-101): diff = ema - w; diff.mul_(1 - decay); ema.sub_(diff) -- three fp32 roundings.
// The files that include this are built with the default contraction mode (changing optim.hip's flags would move AdamW's bits), so
// the mode is switched off for this block alone: `ema - d * omd` as one FMA differs from torch in the last bit.
__device__ __forceinline__ float ema_one(float ema, float p, float one_minus_decay) {
#pragma clang fp contract(off)
    float d = ema - p;
    d = d * one_minus_decay;
    return ema - d;
}

}  // namespace dgs
