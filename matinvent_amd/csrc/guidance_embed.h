// One latent column of the crystal embedding (include/matinvent_hip_guidance.h) for the device and the host alike:
// crystal_embedding_kernel evaluates it per element, scripts/guidance_host_check.cpp holds it to a float64 formula under the host
// sanitizers.  Separately rounded: the units that include it switch contraction off.
#pragma once
#include <math.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace mi {

// (a NaN never gets here: the host turns it into have = 0; both comparisons are false for one, which would hand it on unclamped)
__host__ __device__ inline float guidance_clamp(float yhat) { return yhat < -8.0f ? -8.0f : (yhat > 8.0f ? 8.0f : yhat); }

// sin (cosine = false) or cos (true) of omega * clamp(yhat): |argument| <= 8 (pi / 8) 2^11 = 2048 pi
__host__ __device__ inline float guidance_latent_column(float yhat, float omega, bool cosine) {
    const float arg = omega * guidance_clamp(yhat);
    return cosine ? cosf(arg) : sinf(arg);
}

// column j in [0, Z) of a row with F frequencies per property: which property, which frequency, sine or cosine half
__host__ __device__ inline void guidance_column_index(int j, int F, int* p, int* k, bool* cosine) {
    const int r = j % (2 * F);
    *p = j / (2 * F);
    *cosine = r >= F;
    *k = r >= F ? r - F : r;
}

}  // namespace mi
