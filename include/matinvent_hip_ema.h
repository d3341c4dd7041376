/*
 * matinvent_hip_ema.h -- the fused Adam step with an exponential moving average (EMA) of the weights in the same pass
 * (matinvent_amd.optim.FusedAdam with ema_decay).  Same conventions as matinvent_hip.h (device pointers, fp32, `stream` =
 * hipStream_t as void*, 0 or a negative MI_E* code); a header of its own because the boundary header's entry list is fixed.  The
 * plain step, the gradient norm and the guarded step (matinvent_hip.h, matinvent_hip_optim.h) are untouched: an optimizer without ema_decay
 * never comes here.
 *
 * The weights are one flat fp32 vector and the optimizer is one pass over it, so the average is one more array read and one more array
 * written in that pass: it takes the new weight from the register it was computed in.  For every element
 *
 *     theta, exp_avg, exp_avg_sq   the Adam update of this step (below)
 *     ema = d_s * ema + (1 - d_s) * theta_new                               in float: (1 - d_s) and its product rounded, one fused multiply-add
 *     d_s = ema_warmup ? min(ema_decay, (1 + s) / (10 + s)) : ema_decay     in float64, rounded to float once
 *
 * with s the count of steps this update is the s-th of.  The caller initialises `ema` (FusedAdam: a copy of theta before its first step).
 *
 * state == NULL, the unguarded form: theta, exp_avg and exp_avg_sq get exactly mi_adam_step's arithmetic for the host's step count
 * `step` >= 1, bit for bit; s = step, and d_s is formed on the host.
 * state != NULL, the guarded form: `state` is the state block that the preceding mi_grad_norm on the same stream wrote (same grad, n,
 * grad_scale, beta1, beta2; matinvent_hip_optim.h).  theta, exp_avg and exp_avg_sq get exactly mi_adam_step_guarded's arithmetic, every
 * factor read from the block; `step` and `lr` are ignored.  s is the block's adam_steps -- the applied steps, this one included -- and
 * every wave forms d_s from it: a skipped step does not advance the warm-up.  With apply == 0 nothing is written: theta, exp_avg,
 * exp_avg_sq and ema keep their bits.
 *
 * 16-byte loads and stores when theta, grad, exp_avg, exp_avg_sq and ema are all 16-byte aligned (every torch allocation), dword
 * accesses otherwise; same result.  Vector stores only; no atomics, no scratch memory.
 */
#ifndef MATINVENT_HIP_EMA_H
#define MATINVENT_HIP_EMA_H

#include "matinvent_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n == 0 is MI_OK and enqueues nothing.  Refused with MI_EINVAL before anything is enqueued: a NULL theta / grad / exp_avg / exp_avg_sq /
 * ema, n < 0, an ema_decay outside [0, 1) or NaN, step < 1 in the unguarded form. */
int mi_adam_step_ema(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, int step, float lr, float beta1,
                     float beta2, float eps, float grad_scale, float ema_decay, int ema_warmup, const void* state /* or NULL */, void* stream);

#ifdef __cplusplus
}
#endif

#endif
