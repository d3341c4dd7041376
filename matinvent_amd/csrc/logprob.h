// Per-step scalars and the log-probability terms of the reverse diffusion (diffusion.py:25-29, 297-368), shared by the sampler's recording
// (sampler.hip) and the re-evaluation of a recorded step (traj_logprob.hip), so both compute the same formulas the same way.
// Include after `#pragma clang fp contract(off)`: the arithmetic mirrors the reference's separately-rounded fp32 tensor ops.
// (pymod1, torch's `x % 1.`, lives in common.h.)
#pragma once
#include "common.h"

namespace mi {

struct StepCoef {
    float c0, c1, sigma, sqrt_sn, step_corr, std_corr, step_pred, std_pred, std_corr_sq, std_pred_sq, sigma_sq, log_sigma;
};
__device__ __forceinline__ StepCoef load_coef(const float* coef, int t) {
    const float* c = coef + (size_t)t * MI_NCOEF;
    return StepCoef{c[MI_C_C0], c[MI_C_C1], c[MI_C_SIGMA], c[MI_C_SQRT_SN], c[MI_C_STEP_CORR], c[MI_C_STD_CORR],
                    c[MI_C_STEP_PRED], c[MI_C_STD_PRED], c[MI_C_STD_CORR_SQ], c[MI_C_STD_PRED_SQ], c[MI_C_SIGMA_SQ],
                    c[MI_C_LOG_SIGMA]};
}

// log_prob_wn (diffusion.py:25-29): log sum_{i=-10..10} exp(-(x - mu + i)^2 / 2 / sigma^2)
__device__ __forceinline__ float log_prob_wn(float x, float mu, float sigma_sq) {
    float p = 0.f;
    float d = x - mu;
#pragma unroll
    for (int i = -10; i <= 10; ++i) {
        float v = d + (float)i;
        p += expf(-(v * v) / 2.0f / sigma_sq);
    }
    return logf(p);
}
// torch.distributions.Normal(mu, sigma).log_prob(v)
__device__ __forceinline__ float normal_log_prob(float v, float mu, float var, float log_sigma) {
    float d = v - mu;
    return -(d * d) / (2.0f * var) - log_sigma - 0.91893853320467274178f;
}

// log_prob_wn and its derivative with respect to mu in one pass: returns log p (the same operations, in the same order, as log_prob_wn) and
// *dmu = sum_k w_k (x - mu + k) / sigma^2 / sum_k w_k, w_k = exp(-(x - mu + k)^2 / 2 / sigma^2) -- what torch's autograd of log_prob_wn gives
// (0 / 0 = NaN where the sum underflows, as there)
__device__ __forceinline__ float log_prob_wn_dmu(float x, float mu, float sigma_sq, float* dmu) {
    float p = 0.f, q = 0.f;
    float d = x - mu;
#pragma unroll
    for (int i = -10; i <= 10; ++i) {
        float v = d + (float)i;
        float w = expf(-(v * v) / 2.0f / sigma_sq);
        p += w;
        q += w * (v / sigma_sq);
    }
    *dmu = q / p;
    return logf(p);
}

// sum over a 256-thread block in a fixed tree: the wave sums, then ((w0 + w1) + (w2 + w3)) from `red` (4 floats of LDS) -- the same bits every call
__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum(v);
    int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- predictor (diffusion.py:337-382): the arguments of sampler.hip's predictor_kernel and of its masked form in condition.hip ----
struct PredictorArgs {
    const float *x_mid, *pred_x, *pred_l, *pred_t;
    const float *noise_x, *noise_l, *noise_t;  // slices for step t, or NULL (Philox)
    const float* coef;
    const int* node_off;
    const float* lp_corr;
    float *frac, *lattices, *atom_types;  // state, updated in place
    float *rec_types, *rec_frac, *rec_lat, *rec_lpl, *rec_lpt, *rec_lpx;  // slices (t-1 for state, t for log-probs)
    uint64_t seed;
    int64_t node_offset, graph_offset;
    int t;
    int keep_lattice, keep_coords;  // CSP mode (diffusion.py:283-287, 308-312, 348-349): that part of the state is never moved
};

// the likelihood mask of a conditioned chain (include/matinvent_hip_lik.h): 0 / 1 per atom (types, coordinates) and per crystal (lattice)
struct LikMask {
    const int *known_types, *known_coords, *known_lattice;   // [N], [N], [B]
};

}  // namespace mi
