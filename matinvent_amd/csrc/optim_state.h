// What the guarded Adam (optim.hip) and the Adam with an exponential moving average of the weights (ema.hip) share: the device's state
// block, one element's update and the alignment test of the 16-byte forms.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mi {

// the state block, word by word as include/matinvent_hip_optim.h lists it
struct OptimState {
    float coef, lr_over_bc1, inv_sqrt_bc2;
    unsigned apply, adam_steps, applied, skipped, clipped, nonfinite;
    float last_norm, norm_max;
    unsigned reserved0;
    double norm_sum;
    unsigned reserved1, reserved2;
};
static_assert(sizeof(OptimState) == 64 && offsetof(OptimState, norm_sum) == 48 && offsetof(OptimState, last_norm) == 36, "state block layout");

constexpr int OPT_BLOCK = 256;        // threads per block

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float gscale, float coef, float lr_over_bc1, float inv_sqrt_bc2,
                                         float b1, float b2, float eps) {
    const float gi = g * gscale * coef;   // (coef == 1: adam_kernel's g * gscale, bit for bit)
    const float mi_ = b1 * m + (1.0f - b1) * gi;
    const float vi = b2 * v + (1.0f - b2) * gi * gi;
    m = mi_;
    v = vi;
    p -= lr_over_bc1 * (mi_ / (sqrtf(vi) * inv_sqrt_bc2 + eps));
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace mi
