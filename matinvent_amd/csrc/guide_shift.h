// The arithmetic of mi_guide_seed and mi_guide_shift (include/matinvent_hip_inputgrad.h), host and device: input_grad.hip's
// kernels call these functions, and scripts/guide_host_check.cpp runs the same text against a plain loop under the host sanitizers.
// Separately rounded fp32 operations: no contraction into FMAs.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GUIDE_HD __host__ __device__ inline
#else
#define GUIDE_HD inline
#endif

namespace mi {

enum { GUIDE_MODE_MAX = 0, GUIDE_MODE_MIN = 1, GUIDE_MODE_TARGET = 2 };

#pragma clang fp contract(off)

GUIDE_HD bool guide_finite(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7F800000u) != 0x7F800000u; }   // (false for NaN and +-inf)

// python / torch `x % 1.` (common.h's pymod1, for the host as well)
GUIDE_HD float guide_mod1(float x) {
    float r = x - truncf(x);
    if (r < 0.0f) r += 1.0f;
    return r;
}

// the seed of column p from the predictor's output o (finite)
GUIDE_HD float guide_seed(float o, int mode, float target_hat) {
    return mode == GUIDE_MODE_MAX ? 1.0f : (mode == GUIDE_MODE_MIN ? -1.0f : -(o - target_hat));
}

// a g, clamped elementwise to +-max_shift when max_shift > 0
GUIDE_HD float guide_step(float a, float g, float max_shift) {
    float v = a * g;
    if (max_shift > 0.0f) v = v > max_shift ? max_shift : (v < -max_shift ? -max_shift : v);
    return v;
}

GUIDE_HD float guide_shift_plain(float x, float a, float g, float max_shift) { return x + guide_step(a, g, max_shift); }
GUIDE_HD float guide_shift_wrapped(float x, float a, float g, float max_shift) { return guide_mod1(x + guide_step(a, g, max_shift)); }

// One crystal, serially (the host check's form; the kernel distributes the same element functions over a workgroup): n atoms, the crystal's
// rows.  Returns false -- and writes nothing -- when an element of a given gradient array is not finite.
inline bool guide_shift_crystal_host(int n, int num_types, float* types, float* frac, float* lat, const float* g_types, const float* g_frac,
                                     const float* g_lat, float a_t, float a_x, float a_l, float max_shift) {
    for (int q = 0; q < 9; ++q)
        if (!guide_finite(g_lat[q])) return false;
    for (int i = 0; i < n * 3; ++i)
        if (!guide_finite(g_frac[i])) return false;
    if (g_types)
        for (int i = 0; i < n * num_types; ++i)
            if (!guide_finite(g_types[i])) return false;
    for (int q = 0; q < 9; ++q) lat[q] = guide_shift_plain(lat[q], a_l, g_lat[q], max_shift);
    for (int i = 0; i < n * 3; ++i) frac[i] = guide_shift_wrapped(frac[i], a_x, g_frac[i], max_shift);
    if (g_types)
        for (int i = 0; i < n * num_types; ++i) types[i] = guide_shift_plain(types[i], a_t, g_types[i], max_shift);
    return true;
}

}  // namespace mi
