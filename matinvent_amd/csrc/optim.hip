// Global-norm gradient clipping and the non-finite-step guard of the fused Adam (include/matinvent_hip_optim.h):
//   grad_sumsq_kernel   sum of (grad[i] * grad_scale)^2 per block, in float64, to the workspace (plain stores, fixed order: same bits every call)
//   grad_finish_kernel  one block: adds the per-block sums in a fixed order; norm, clipping coefficient, apply flag, the applied step's
//                       bias-corrected step size and the running statistics -> the state block
//   adam_guarded_kernel adam_kernel's arithmetic (backward.hip) with g = grad * grad_scale * coef, 16 bytes per lane; writes nothing
//                       when the state block's apply flag is clear
// The three launches of a step follow each other on one stream: each reads what the one before wrote across a launch boundary, so there
// is no in-launch hand-off, no fence and no counter to re-arm.
#include <math.h>
#include <stddef.h>

#include "../../include/matinvent_hip_optim.h"
#include "common.h"
#include "optim_state.h"

namespace mi {

constexpr int OPT_UNROLL = 4;         // 16-byte loads in flight per thread and sweep
constexpr int OPT_MAX_BLOCKS = 2048;  // 8 blocks on each of 256 CUs: fills the chip, the rest is grid-stride
constexpr int64_t OPT_BLOCK_ELEMS = (int64_t)OPT_BLOCK * OPT_UNROLL * 4;   // elements of one block in one sweep

// the grid of the reduction: a function of n alone
static int optim_blocks(int64_t n) {
    int64_t b = (n + OPT_BLOCK_ELEMS - 1) / OPT_BLOCK_ELEMS;
    return (int)(b < 1 ? 1 : b > OPT_MAX_BLOCKS ? OPT_MAX_BLOCKS : b);
}

// Sum over the block of one double per thread, in a fixed tree; valid in thread 0.  `red`: 4 doubles of LDS.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ double sq64(float g, double scale) {
    const double x = (double)g * scale;   // exact: 24 x 24 significant bits
    return x * x;
}

// VEC: grad is 16-byte aligned and read as float4 (unit = 4 elements); otherwise dword loads (unit = 1 element).  Unit u of sweep s, slot c
// belongs to global thread ((s * OPT_UNROLL + c) * threads + thread): consecutive lanes read consecutive units.  The n % 4 elements behind
// the last whole float4 belong to thread 0 of block 0.
template <bool VEC>
__global__ __launch_bounds__(OPT_BLOCK) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n, float grad_scale, double* __restrict__ partial) {
    __shared__ double red[4];
    const double scale = (double)grad_scale;
    const int64_t threads = (int64_t)gridDim.x * OPT_BLOCK, tid = (int64_t)blockIdx.x * OPT_BLOCK + threadIdx.x;
    const int64_t units = VEC ? n / 4 : n;
    double acc = 0.0;
    for (int64_t u0 = tid; u0 < units; u0 += threads * OPT_UNROLL) {
        if constexpr (VEC) {
            const float4* g4 = reinterpret_cast<const float4*>(g);
            float4 v[OPT_UNROLL];
#pragma unroll
            for (int c = 0; c < OPT_UNROLL; ++c) {
                const int64_t u = u0 + c * threads;
                v[c] = u < units ? g4[u] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int c = 0; c < OPT_UNROLL; ++c) acc += (sq64(v[c].x, scale) + sq64(v[c].y, scale)) + (sq64(v[c].z, scale) + sq64(v[c].w, scale));
        } else {
            float v[OPT_UNROLL];
#pragma unroll
            for (int c = 0; c < OPT_UNROLL; ++c) {
                const int64_t u = u0 + c * threads;
                v[c] = u < units ? g[u] : 0.f;
            }
#pragma unroll
            for (int c = 0; c < OPT_UNROLL; ++c) acc += sq64(v[c], scale);
        }
    }
    if (VEC && tid == 0)
        for (int64_t i = units * 4; i < n; ++i) acc += sq64(g[i], scale);
    const double s = block_sum_f64(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

struct FinishArgs {
    float max_norm, lr, beta1, beta2;
    int skip_nonfinite, nblocks;
};

__global__ __launch_bounds__(OPT_BLOCK) void grad_finish_kernel(const double* __restrict__ partial, FinishArgs a, OptimState* __restrict__ st) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < a.nblocks; i += OPT_BLOCK) acc += partial[i];
    const double sum = block_sum_f64(acc, red);
    if (threadIdx.x != 0) return;
    const float norm = (float)sqrt(sum);
    const bool finite = isfinite(norm);
    float coef = 1.0f;
    if (a.max_norm > 0.f) {   // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1.0), NaN kept
        const float c = a.max_norm / (norm + 1e-6f);
        coef = c < 1.0f ? c : (c != c ? c : 1.0f);
    }
    const bool apply = finite || !a.skip_nonfinite;
    st->coef = coef;
    st->apply = apply ? 1u : 0u;
    if (apply) {
        const unsigned s = st->adam_steps + 1u;
        const double bc1 = 1.0 - pow((double)a.beta1, (double)s), bc2 = 1.0 - pow((double)a.beta2, (double)s);
        st->lr_over_bc1 = (float)((double)a.lr / bc1);
        st->inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
        st->adam_steps = s;
        st->applied += 1u;
        if (finite && coef < 1.0f) st->clipped += 1u;
    } else {
        st->skipped += 1u;
    }
    st->last_norm = norm;
    if (finite) {
        st->norm_sum += (double)norm;
        st->norm_max = fmaxf(st->norm_max, norm);
    } else {
        st->nonfinite += 1u;
    }
}

// Item i < units: elements 4 i .. 4 i + 3 (VEC) or element i; with VEC, item `units` is the n % 4 elements behind the last whole float4.
template <bool VEC>
__global__ __launch_bounds__(OPT_BLOCK) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                 float* __restrict__ v, int64_t n, const OptimState* __restrict__ st, float b1, float b2,
                                                                 float eps, float gscale) {
    // wave-uniform: the same four words for every lane (a scalar load, or one lane's value broadcast)
    if (__builtin_amdgcn_readfirstlane(st->apply) == 0u) return;
    const float coef = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, st->coef)));
    const float lr_over_bc1 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, st->lr_over_bc1)));
    const float inv_sqrt_bc2 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, st->inv_sqrt_bc2)));
    const int64_t i = (int64_t)blockIdx.x * OPT_BLOCK + threadIdx.x;
    const int64_t units = VEC ? n / 4 : n;
    if (i < units) {
        if constexpr (VEC) {
            float4 pp = reinterpret_cast<float4*>(p)[i], mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
            const float4 gg = reinterpret_cast<const float4*>(g)[i];
            adam_one(pp.x, gg.x, mm.x, vv.x, gscale, coef, lr_over_bc1, inv_sqrt_bc2, b1, b2, eps);
            adam_one(pp.y, gg.y, mm.y, vv.y, gscale, coef, lr_over_bc1, inv_sqrt_bc2, b1, b2, eps);
            adam_one(pp.z, gg.z, mm.z, vv.z, gscale, coef, lr_over_bc1, inv_sqrt_bc2, b1, b2, eps);
            adam_one(pp.w, gg.w, mm.w, vv.w, gscale, coef, lr_over_bc1, inv_sqrt_bc2, b1, b2, eps);
            reinterpret_cast<float4*>(m)[i] = mm;
            reinterpret_cast<float4*>(v)[i] = vv;
            reinterpret_cast<float4*>(p)[i] = pp;
        } else {
            adam_one(p[i], g[i], m[i], v[i], gscale, coef, lr_over_bc1, inv_sqrt_bc2, b1, b2, eps);
        }
    } else if (VEC && i == units) {
        for (int64_t k = units * 4; k < n; ++k) adam_one(p[k], g[k], m[k], v[k], gscale, coef, lr_over_bc1, inv_sqrt_bc2, b1, b2, eps);
    }
}

}  // namespace mi

using namespace mi;

extern "C" {

int64_t mi_optim_state_bytes(void) { return (int64_t)sizeof(OptimState); }

int64_t mi_optim_workspace_bytes(int64_t n) {
    MI_CHECK(n >= 0, MI_EINVAL, "mi_optim_workspace_bytes: n = %lld", (long long)n);
    return (int64_t)optim_blocks(n) * (int64_t)sizeof(double);
}

int64_t mi_optim_sweep_elems(int64_t n) {
    MI_CHECK(n >= 0, MI_EINVAL, "mi_optim_sweep_elems: n = %lld", (long long)n);
    return (int64_t)optim_blocks(n) * OPT_BLOCK_ELEMS;
}

int mi_grad_norm(const float* grad, int64_t n, float grad_scale, float max_norm, int skip_nonfinite, float lr, float beta1, float beta2,
                 void* state, void* workspace, void* stream) {
    MI_CHECK(grad && state && workspace, MI_EINVAL, "mi_grad_norm: null argument");
    MI_CHECK(n >= 0, MI_EINVAL, "mi_grad_norm: n = %lld", (long long)n);
    MI_CHECK(max_norm == max_norm, MI_EINVAL, "mi_grad_norm: max_norm is NaN");
    MI_CHECK(((uintptr_t)state & 15u) == 0 && ((uintptr_t)workspace & 7u) == 0, MI_EINVAL, "mi_grad_norm: state / workspace alignment");
    const int blocks = n > 0 ? optim_blocks(n) : 0;
    if (blocks) {
        if (aligned16(grad))
            hipLaunchKernelGGL(grad_sumsq_kernel<true>, dim3(blocks), dim3(OPT_BLOCK), 0, (hipStream_t)stream, grad, n, grad_scale, (double*)workspace);
        else
            hipLaunchKernelGGL(grad_sumsq_kernel<false>, dim3(blocks), dim3(OPT_BLOCK), 0, (hipStream_t)stream, grad, n, grad_scale, (double*)workspace);
        MI_KERNEL_CHECK();
    }
    FinishArgs a{max_norm, lr, beta1, beta2, skip_nonfinite ? 1 : 0, blocks};
    hipLaunchKernelGGL(grad_finish_kernel, dim3(1), dim3(OPT_BLOCK), 0, (hipStream_t)stream, (const double*)workspace, a, (OptimState*)state);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int mi_adam_step_guarded(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1, float beta2, float eps,
                         float grad_scale, const void* state, void* stream) {
    MI_CHECK(theta && grad && exp_avg && exp_avg_sq && state, MI_EINVAL, "mi_adam_step_guarded: null argument");
    MI_CHECK(n >= 0, MI_EINVAL, "mi_adam_step_guarded: n = %lld", (long long)n);
    if (n == 0) return MI_OK;
    if (aligned16(theta) && aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq)) {
        const int64_t items = n / 4 + (n % 4 ? 1 : 0);
        hipLaunchKernelGGL(adam_guarded_kernel<true>, dim3((unsigned)cdiv(items, OPT_BLOCK)), dim3(OPT_BLOCK), 0, (hipStream_t)stream, theta, grad,
                           exp_avg, exp_avg_sq, n, (const OptimState*)state, beta1, beta2, eps, grad_scale);
    } else {
        hipLaunchKernelGGL(adam_guarded_kernel<false>, dim3((unsigned)cdiv(n, OPT_BLOCK)), dim3(OPT_BLOCK), 0, (hipStream_t)stream, theta, grad,
                           exp_avg, exp_avg_sq, n, (const OptimState*)state, beta1, beta2, eps, grad_scale);
    }
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // extern "C"
