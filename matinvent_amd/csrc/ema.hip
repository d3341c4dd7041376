// The fused Adam with an exponential moving average of the weights in the same pass (include/matinvent_hip_ema.h):
//   adam_ema_kernel<VEC, GUARDED>  adam_guarded_kernel's shape (optim.hip): 256 threads, 16 bytes per lane and array when all five pointers
//                                  are 16-byte aligned (one item for the n % 4 tail), dword loads otherwise.  One element's Adam update is
//                                  adam_one's (optim_state.h) with its fused multiply-adds written out (adam_one_stated below); the
//                                  average reads the freshly computed weight from the register it was computed in.
//   GUARDED  every factor from the state block the preceding mi_grad_norm wrote, read once per wave; the decay from its adam_steps
//            (ema_decay.h), per wave; nothing is written, the average included, when the apply flag is clear.
//   else     the factors and the decay are formed on the host for the host's step count, as mi_adam_step forms them; coef = 1.
// Plain vector stores only: no atomics, no LDS, no scratch.
#include <math.h>

#include "../../include/matinvent_hip_ema.h"
#include "common.h"
#include "ema_decay.h"
#include "optim_state.h"

namespace mi {

struct AdamEmaArgs {
    float* p;
    const float* g;
    float *m, *v, *e;
    int64_t n;
    const OptimState* st;                       // GUARDED only
    float b1, b2, eps, gscale;
    float lr_over_bc1, inv_sqrt_bc2, decay;     // unguarded: this step's factors and d_s.  GUARDED: decay = ema_decay, the others unused
    int warmup;                                 // GUARDED only
};

// adam_one (optim_state.h) leaves the choice of fused multiply-adds to the compiler.  In adam_kernel and in both adam_guarded_kernel forms
// it fuses b1 * m, b2 * v, sqrt(v) * inv_sqrt_bc2 and lr_over_bc1 * q into the additions behind them and rounds the other product of
// each sum on its own (profiles/ema_isa_compare.txt has their code).  With one more consumer of the new weight it chose otherwise here
// -- the other product of the two moment sums -- and the moments' last bits moved.  So this kernel states those four operations, with
// contraction off for everything else: theta, exp_avg and exp_avg_sq are the two other kernels' bit for bit, which the tests hold it to.
__device__ __forceinline__ void adam_one_stated(float& p, float g, float& m, float& v, float gscale, float coef, float lr_over_bc1,
                                                float inv_sqrt_bc2, float b1, float b2, float eps) {
#pragma clang fp contract(off)
    const float gi = g * gscale * coef;   // (coef == 1: g * gscale)
    const float mi_ = __builtin_fmaf(b1, m, (1.0f - b1) * gi);
    const float vi = __builtin_fmaf(b2, v, (1.0f - b2) * gi * gi);
    m = mi_;
    v = vi;
    p = __builtin_fmaf(-(mi_ / __builtin_fmaf(sqrtf(vi), inv_sqrt_bc2, eps)), lr_over_bc1, p);
}

// ema = d * ema + (1 - d) * theta_new in float: omd = 1.0f - d, the product omd * theta_new rounded, then one fused multiply-add
__device__ __forceinline__ void ema_one(float& e, float p, float d, float omd) {
#pragma clang fp contract(off)
    e = __builtin_fmaf(d, e, omd * p);
}

__device__ __forceinline__ float uniform_f32(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, x)));
}

template <bool VEC, bool GUARDED>
__global__ __launch_bounds__(OPT_BLOCK) void adam_ema_kernel(AdamEmaArgs a) {
    float coef = 1.0f, lr_over_bc1 = a.lr_over_bc1, inv_sqrt_bc2 = a.inv_sqrt_bc2, d = a.decay;
    if constexpr (GUARDED) {
        // wave-uniform: the same five words for every lane (a scalar load, or one lane's value broadcast)
        if (__builtin_amdgcn_readfirstlane(a.st->apply) == 0u) return;
        coef = uniform_f32(a.st->coef);
        lr_over_bc1 = uniform_f32(a.st->lr_over_bc1);
        inv_sqrt_bc2 = uniform_f32(a.st->inv_sqrt_bc2);
        d = ema_decay_at(a.decay, a.warmup, __builtin_amdgcn_readfirstlane(a.st->adam_steps));   // (applied steps, this one included)
    }
    const float omd = 1.0f - d;
    float* __restrict__ p = a.p;
    const float* __restrict__ g = a.g;
    float* __restrict__ m = a.m;
    float* __restrict__ v = a.v;
    float* __restrict__ e = a.e;
    const int64_t n = a.n;
    const int64_t i = (int64_t)blockIdx.x * OPT_BLOCK + threadIdx.x;
    const int64_t units = VEC ? n / 4 : n;
    if (i < units) {
        if constexpr (VEC) {
            float4 pp = reinterpret_cast<float4*>(p)[i], mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
            float4 ee = reinterpret_cast<float4*>(e)[i];
            const float4 gg = reinterpret_cast<const float4*>(g)[i];
            adam_one_stated(pp.x, gg.x, mm.x, vv.x, a.gscale, coef, lr_over_bc1, inv_sqrt_bc2, a.b1, a.b2, a.eps);
            adam_one_stated(pp.y, gg.y, mm.y, vv.y, a.gscale, coef, lr_over_bc1, inv_sqrt_bc2, a.b1, a.b2, a.eps);
            adam_one_stated(pp.z, gg.z, mm.z, vv.z, a.gscale, coef, lr_over_bc1, inv_sqrt_bc2, a.b1, a.b2, a.eps);
            adam_one_stated(pp.w, gg.w, mm.w, vv.w, a.gscale, coef, lr_over_bc1, inv_sqrt_bc2, a.b1, a.b2, a.eps);
            ema_one(ee.x, pp.x, d, omd);
            ema_one(ee.y, pp.y, d, omd);
            ema_one(ee.z, pp.z, d, omd);
            ema_one(ee.w, pp.w, d, omd);
            reinterpret_cast<float4*>(m)[i] = mm;
            reinterpret_cast<float4*>(v)[i] = vv;
            reinterpret_cast<float4*>(p)[i] = pp;
            reinterpret_cast<float4*>(e)[i] = ee;
        } else {
            adam_one_stated(p[i], g[i], m[i], v[i], a.gscale, coef, lr_over_bc1, inv_sqrt_bc2, a.b1, a.b2, a.eps);
            ema_one(e[i], p[i], d, omd);
        }
    } else if (VEC && i == units) {   // the n % 4 elements behind the last whole float4
        for (int64_t k = units * 4; k < n; ++k) {
            adam_one_stated(p[k], g[k], m[k], v[k], a.gscale, coef, lr_over_bc1, inv_sqrt_bc2, a.b1, a.b2, a.eps);
            ema_one(e[k], p[k], d, omd);
        }
    }
}

template <bool GUARDED>
static int launch_adam_ema(const AdamEmaArgs& a, hipStream_t stream) {
    if (aligned16(a.p) && aligned16(a.g) && aligned16(a.m) && aligned16(a.v) && aligned16(a.e)) {
        const int64_t items = a.n / 4 + (a.n % 4 ? 1 : 0);
        hipLaunchKernelGGL((adam_ema_kernel<true, GUARDED>), dim3((unsigned)cdiv(items, OPT_BLOCK)), dim3(OPT_BLOCK), 0, stream, a);
    } else {
        hipLaunchKernelGGL((adam_ema_kernel<false, GUARDED>), dim3((unsigned)cdiv(a.n, OPT_BLOCK)), dim3(OPT_BLOCK), 0, stream, a);
    }
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_adam_step_ema(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, int step, float lr, float beta1,
                     float beta2, float eps, float grad_scale, float ema_decay, int ema_warmup, const void* state, void* stream) {
    MI_CHECK(theta && grad && exp_avg && exp_avg_sq && ema, MI_EINVAL, "mi_adam_step_ema: null argument");
    MI_CHECK(n >= 0, MI_EINVAL, "mi_adam_step_ema: n = %lld", (long long)n);
    MI_CHECK(ema_decay >= 0.0f && ema_decay < 1.0f, MI_EINVAL, "mi_adam_step_ema: ema_decay = %g lies outside [0, 1)", (double)ema_decay);
    MI_CHECK(state || step >= 1, MI_EINVAL, "mi_adam_step_ema: step = %d (the unguarded form counts from 1)", step);
    if (n == 0) return MI_OK;
    AdamEmaArgs a{theta, grad, exp_avg, exp_avg_sq, ema, n, (const OptimState*)state, beta1, beta2, eps, grad_scale, 0.f, 0.f, ema_decay,
                  ema_warmup ? 1 : 0};
    if (state) return launch_adam_ema<true>(a, (hipStream_t)stream);
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);   // mi_adam_step's, to the letter
    a.lr_over_bc1 = (float)(lr / bc1);
    a.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    a.decay = ema_decay_at(ema_decay, ema_warmup, (unsigned)step);
    return launch_adam_ema<false>(a, (hipStream_t)stream);
}

}  // extern "C"
