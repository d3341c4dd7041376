// The resampling plan of one particle group (include/matinvent_hip_steer.h): scores, log-weights, effective sample size and the
// systematic resampling's ancestors, as plain sequential text for the host and the device alike.  steer.hip's plan kernel runs it on one
// thread of the group's workgroup over arrays in LDS; scripts/steer_host_check.cpp compiles it for the host and holds it to a plain loop
// under the host sanitizers; tests/steer_ref.py restates it in float64.
//
// THE ORDER, fixed here: every sum runs over k = 0, 1, ..., K - 1 in that order in fp32 (S = sum w, Q = sum w^2, and the cumulative sums
// c_k = w_0 + ... + w_k, so that c_{K-1} and S are the same bits); the thresholds are t_j = ((U + (float)j) / (float)K) * S for
// j = 0 .. K - 1, and offspring j takes the smallest k with c_k > t_j (never an index behind the last particle of non-zero weight: the
// guard of a threshold that rounds up to S).  Separately rounded operations: no contraction into FMAs.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MI_STEER_HD __host__ __device__ __forceinline__
#else
#define MI_STEER_HD inline
#endif

namespace mi {

constexpr int STEER_MAX_K = 256;                                       // particles per group (MI_STEER_MAX_PARTICLES)
constexpr int STEER_MODE_MAX = 0, STEER_MODE_MIN = 1, STEER_MODE_TARGET = 2;
constexpr int STEER_RESAMPLED = 1, STEER_NO_FINITE = 2;                // steer_plan_group's return bits

#pragma clang fp contract(off)

MI_STEER_HD bool steer_finite(float v) {
    return (__builtin_bit_cast(uint32_t, v) & 0x7F800000u) != 0x7F800000u;
}

// u = +o (max), -o (min), -|o - target| (target)
MI_STEER_HD float steer_score(float o, int mode, float target) {
    if (mode == STEER_MODE_MAX) return o;
    if (mode == STEER_MODE_MIN) return -o;
    return -fabsf(o - target);
}

// lw = logw + lambda (u - u_prev); a particle whose score is not finite, or whose log-weight comes out as NaN (its previous score was not
// finite and it has not been resampled since), has weight 0: lw = -inf.  +inf is clamped to the largest float.
MI_STEER_HD float steer_logweight(float logw, float lambda, float u, float u_prev) {
    const float d = u - u_prev;
    const float s = lambda * d;
    float lw = logw + s;
    if (!steer_finite(u) || lw != lw) return -INFINITY;
    if (lw > 3.402823466e+38f) lw = 3.402823466e+38f;
    return lw;
}

// One group.  In: K, u[K] the scores of this level, lw[K] the log-weights of this level (steer_logweight), U in [0, 1).  Scratch: w[K].
// Out: anc[K] (indices 0 .. K - 1 inside the group), u_prev[K] and logw[K] as the header states, *ess (0 for a group without weight).
// Returns STEER_RESAMPLED and / or STEER_NO_FINITE.
MI_STEER_HD int steer_plan_group(int K, const float* u, const float* lw, float ess_frac, float U, float* w, int* anc, float* u_prev, float* logw,
                                 float* ess) {
    float m = -INFINITY;
    for (int k = 0; k < K; ++k) m = lw[k] > m ? lw[k] : m;
    for (int k = 0; k < K; ++k) anc[k] = k;
    *ess = 0.f;
    if (m == -INFINITY) return STEER_NO_FINITE;   // no particle of finite weight: the identity, u_prev and logw stay what they were
    float S = 0.f, Q = 0.f;
    int last = 0;
    bool equal = true;
    for (int k = 0; k < K; ++k) {
        const float d = lw[k] - m;
        const float v = lw[k] == -INFINITY ? 0.f : expf(d);
        w[k] = v;
        S = S + v;
        const float v2 = v * v;
        Q = Q + v2;
        if (v > 0.f) last = k;
        if (__builtin_bit_cast(uint32_t, v) != __builtin_bit_cast(uint32_t, w[0])) equal = false;
    }
    const float S2 = S * S;
    const float e = S2 / Q;
    *ess = e;
    const float limit = ess_frac * (float)K;
    const bool resample = ess_frac < 0.f || e < limit;
    if (!resample) {
        for (int k = 0; k < K; ++k) {
            u_prev[k] = u[k];
            logw[k] = lw[k];
        }
        return 0;
    }
    if (!equal) {   // (bit-equal weights: the identity set above, by construction)
        float c = w[0];
        int k = 0;
        for (int j = 0; j < K; ++j) {
            const float a = U + (float)j;
            const float f = a / (float)K;
            const float t = f * S;
            while (k < last && !(c > t)) {
                ++k;
                c = c + w[k];
            }
            anc[j] = k;
        }
    }
    for (int k = 0; k < K; ++k) logw[k] = 0.f;
    // u_prev_k = u_{a_k}: u is not overwritten, so the order of these writes does not matter
    for (int k = 0; k < K; ++k) u_prev[k] = u[anc[k]];
    return STEER_RESAMPLED;
}

}  // namespace mi
