/*
 * matinvent_hip_optim.h -- global-norm gradient clipping and a non-finite-step guard for the fused Adam on the flat parameter vector
 * (matinvent_amd.optim.FusedAdam with max_grad_norm / skip_nonfinite).  Same conventions as matinvent_hip.h (device pointers,
 * fp32, `stream` = hipStream_t as void*, 0 or a negative MI_E* code); a header of its own because the boundary header's entry list is
 * fixed.  mi_adam_step (matinvent_hip.h) is untouched: an optimizer that uses neither option never comes here.
 *
 * One optimizer step is two calls on one stream, neither of which synchronises the host:
 *   mi_grad_norm          norm = sqrt(sum_i (grad[i] * grad_scale)^2), the clipping coefficient, the decision whether the step is applied,
 *                         the step size of the applied step and the running statistics -> the STATE BLOCK (device memory);
 *   mi_adam_step_guarded  mi_adam_step's update with g = grad * grad_scale * coef, every factor read from the state block; a step that is
 *                         not applied writes nothing.
 * A skipped step must not advance Adam's bias corrections, and the host cannot know that a step was skipped without waiting for the device:
 * so the count of APPLIED steps lives in the state block, and lr / (1 - beta1^s), 1 / sqrt(1 - beta2^s) are formed on the device for
 * s = that count + 1 (in float64, rounded to float once, as mi_adam_step forms them on the host).
 *
 * THE STATE BLOCK: mi_optim_state_bytes() = 64 bytes = 16 four-byte words, 16-byte aligned, ZEROED by the caller before the first step
 * (hipMemset / torch.zeros) and owned by the device from then on.  Word by word (u32 = unsigned 32-bit, f32 = float, f64 = double):
 *    0  f32  coef           clipping coefficient of the last step: min(1, max_norm / (norm + 1e-6)), computed in float like
 *                           torch.nn.utils.clip_grad_norm_; exactly 1.0 when clipping is off or the norm is below max_norm; NaN when the norm is
 *    1  f32  lr_over_bc1    lr / (1 - beta1^s) of the last APPLIED step
 *    2  f32  inv_sqrt_bc2   1 / sqrt(1 - beta2^s) of the last APPLIED step
 *    3  u32  apply          1: mi_adam_step_guarded applies the last step; 0: it writes nothing.  = isfinite(norm) || !skip_nonfinite
 *    4  u32  adam_steps     s: steps applied since the block was zeroed (Adam's bias-correction count).  Never reset by a statistics reset.
 *    5  u32  applied        statistics: steps applied ...
 *    6  u32  skipped        ... steps skipped (non-finite norm with skip_nonfinite) ...
 *    7  u32  clipped        ... applied steps with coef < 1 ...
 *    8  u32  nonfinite      ... steps whose norm was inf or NaN, skipped or not
 *    9  f32  last_norm      norm of the last step (before clipping), whatever it was
 *   10  f32  norm_max       largest finite norm
 *   11  u32  (reserved, 0)
 *   12  f64  norm_sum       sum of the finite norms (words 12-13): the mean norm is norm_sum / (applied + skipped - nonfinite)
 *   14  u32  (reserved, 0)
 *   15  u32  (reserved, 0)
 * Words 5 .. 13 are statistics only: the caller may zero them between steps (on the same stream) to start a new period.
 *
 * The sum of squares is bit-reproducible: the grid is a function of n alone (mi_optim_sweep_elems), every element belongs to a fixed thread,
 * every thread, wave and block adds in a fixed order, the per-block sums go to `workspace` by plain stores and are added in a fixed order
 * by one block; there are no atomics.  Every product and every sum is float64 (the product grad[i] * grad_scale exactly), so no square
 * overflows or underflows for any finite float; the norm is rounded to float once (relative 2^-24 + n 2^-53).  A norm beyond FLT_MAX, and
 * any inf / NaN element, give a non-finite norm: the step is skipped (skip_nonfinite) or applied as it stands.
 */
#ifndef MATINVENT_HIP_OPTIM_H
#define MATINVENT_HIP_OPTIM_H

#include "matinvent_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only (no device needed). */
int64_t mi_optim_state_bytes(void);               /* the state block: 64 */
int64_t mi_optim_workspace_bytes(int64_t n);      /* per-block partial sums of the reduction over n elements (n < 0: MI_EINVAL) */
int64_t mi_optim_sweep_elems(int64_t n);          /* elements the grid chosen for n covers in one grid-stride sweep (n < 0: MI_EINVAL) */

/* mi_grad_norm: the reduction over grad[0 .. n) and the finishing step of ONE optimizer step (see above).
 *   max_norm: > 0 clips to that global norm (+inf: never clips); <= 0: no clipping, coef = 1, the norm is reported only.
 *   skip_nonfinite: non-zero -> a step with a non-finite norm is not applied.
 *   lr, beta1, beta2: Adam's, for the step size of the applied step (words 1-2 of the state block).
 *   state: the state block.  workspace: mi_optim_workspace_bytes(n) bytes, 8-byte aligned; free for reuse when the call's kernels are done.
 * 16-byte loads when grad is 16-byte aligned (every torch allocation), dword loads otherwise; same result.
 * n == 0 is a step with norm 0 (applied).  Refused with MI_EINVAL before anything is enqueued: a NULL grad / state / workspace, n < 0,
 * a NaN max_norm. */
int mi_grad_norm(const float* grad, int64_t n, float grad_scale, float max_norm, int skip_nonfinite, float lr, float beta1, float beta2,
                 void* state, void* workspace, void* stream);

/* mi_adam_step_guarded: mi_adam_step's arithmetic with g = grad[i] * grad_scale * coef and the step size of the state block, which the
 * preceding mi_grad_norm on the same stream wrote (same grad, n, grad_scale, beta1, beta2).  With apply == 0 theta, exp_avg and exp_avg_sq
 * keep their bits.  Refused with MI_EINVAL before anything is enqueued: a NULL pointer, n < 0. */
int mi_adam_step_guarded(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1, float beta2, float eps,
                         float grad_scale, const void* state, void* stream);

#ifdef __cplusplus
}
#endif

#endif
