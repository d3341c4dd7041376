/*
 * matinvent_hip_pg.h -- policy-gradient extension of the trajectory ABI (include/matinvent_hip_traj.h): one fused micro-step of the
 * PPO-clipped surrogate on recorded trajectories (matinvent_amd.policy.pg_step).  Same conventions as matinvent_hip.h (device pointers
 * unless a name ends in `_host`, fp32, int32 indices, row-major, `stream` = hipStream_t as void*, 0 or a negative MI_E* code); a header of
 * its own because the trajectory header's entry list is fixed.
 */
#ifndef MATINVENT_HIP_PG_H
#define MATINVENT_HIP_PG_H

#include "matinvent_hip_traj.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mi_traj_pg_step: one micro-step of the PPO-clipped policy gradient on recorded trajectories (matinvent_amd.policy.pg_step), enqueued
 * on `stream` without a host synchronisation.  The rollout holds the kept crystals' whole chains, stacked over t = 0..T:
 *   traj_atom_types [T+1][N][A], traj_frac / traj_frac_mid [T+1][N][3], traj_lattices [T+1][B][9],
 *   traj_lp_old [T+1][B][3] = the sampler's recorded { log_prob_l, log_prob_t, log_prob_x }
 * over the atom counts of (b_corr, b_pred).  Crystal b is evaluated at ITS time t_b: t_host [B] (host; each in 2..T, else MI_EINVAL before
 * anything is enqueued) and t_dev [B] (the same values on the device -- the kernels read these; nothing is read back).
 *   1. one gather launch writes crystal b's state at t_b and t_b - 1 (the seven inputs of mi_traj_logprob) into b_corr's buffers;
 *   2. mi_traj_logprob's two taped evaluations and its log-probability kernel;
 *   3. one surrogate launch, one thread per crystal: lp_new = w . (lp_l, lp_t, lp_x), lp_old = w . traj_lp_old[t_b][b],
 *      rho = exp(lp_new - lp_old), L_b = max(-A_b rho, -A_b clip(rho, 1 - eps, 1 + eps)) (adv_dev [B] = A), and the upstream gradient
 *      g_b = (loss_scale * -A_b) * rho where the unclipped term is selected (rho in [1 - eps, 1 + eps], or the unclipped term strictly
 *      larger), 0 otherwise; seeds w_k g_b.  stats [4][B] ACCUMULATES (+=) L_b, rho, (lp_new - lp_old)^2 / 2 and [|rho - 1| > eps];
 *   4. mi_traj_logprob_backward with those seeds: grad_theta += d(sum_b L_b * loss_scale) / d theta.
 * w_host [3]: the log-probability weights (host); log_prob [3][B]: optional copy of the new log-probabilities (NULL: not kept). */
int mi_traj_pg_step(mi_net* net, mi_batch* b_corr, mi_batch* b_pred, const float* coef_dev, int T, const float* time_freqs,
                    const float* traj_atom_types, const float* traj_frac, const float* traj_frac_mid, const float* traj_lattices,
                    const float* traj_lp_old, const int* t_host, const int* t_dev, const float* adv_dev, float clip_range,
                    const float* w_host, float loss_scale, float* log_prob, float* grad_theta, float* stats, void* stream);

#ifdef __cplusplus
}
#endif

#endif
