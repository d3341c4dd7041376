/*
 * matinvent_hip_pg_kl.h -- the policy-gradient micro-step of include/matinvent_hip_pg.h with a per-step KL anchor to a frozen prior network
 * (matinvent_amd.policy.pg_step with kl_coef > 0).  Same conventions as matinvent_hip.h (device pointers unless a name ends in `_host`, fp32,
 * int32 indices, row-major, `stream` = hipStream_t as void*, 0 or a negative MI_E* code); a header of its own because the policy-gradient
 * header's entry list is fixed.
 */
#ifndef MATINVENT_HIP_PG_KL_H
#define MATINVENT_HIP_PG_KL_H

#include "matinvent_hip_pg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mi_traj_pg_kl_step: mi_traj_pg_step (same arguments, same meaning) plus beta * KL_b per crystal, where
 *   KL_b = w . (KL_l, KL_t, KL_x),  KL_k = KL( p_theta(x_{t-1} | x_t) || p_prior(x_{t-1} | x_t) ) of term k at crystal b's time t_b,
 * averaged like the matching log-probability.  Every transition is a Normal (lattice, types) or a wrapped Normal (coordinates) whose variance
 * does not depend on the network, so KL_k is a closed form in the difference of the two networks' predictions (coordinates: the unwrapped
 * KL at the nearest image, an upper bound of the wrapped one):
 *   KL_l = 1/9 sum (c0 c1 (pl_a - pl_p))^2 / (2 sigma^2)          KL_t = 1/n sum_atoms 1/100 sum (c0 c1 (pt_a - pt_p))^2 / (2 sigma^2)
 *   KL_x = 1/(3n) sum mi(step_corr sqrt(sn) (pxc_a - pxc_p))^2 / (2 std_corr^2) + 1/(3n) sum mi(step_pred sqrt(sn) (pxp_a - pxp_p))^2 / (2 std_pred^2)
 * with mi(d) = d - rint(d), pl / pt / pxp the predictor evaluation's heads and pxc the corrector evaluation's coordinate head.
 *   prior, b_prior: the frozen network and ONE inference batch handle of it over the atom counts of (b_corr, b_pred), used for both of the
 *     prior's evaluations (corrector and predictor input; no tape).  With aux_stream non-NULL and != stream they run on aux_stream, forked
 *     after the gather and joined before the KL kernel; otherwise on `stream`, before the agent's evaluations.
 *   kl_coef: beta >= 0.  grad_theta += d(sum_b (L_b + beta KL_b) * loss_scale) / d theta (the agent's parameters only).
 *   stats [5][B]: rows 0..3 as mi_traj_pg_step's; row 4 ACCUMULATES (+=) KL_b (weighted by w, not by beta).
 *   kl_out [3][B]: optional copy of (KL_l, KL_t, KL_x) of this call (NULL: not kept).
 * Refused with MI_EINVAL before anything is enqueued: whatever mi_traj_pg_step refuses, a NULL prior or b_prior, b_prior created for another
 * network or equal to b_corr / b_pred, other atom counts than b_corr's, kl_coef < 0 (or NaN).  No host synchronisation. */
int mi_traj_pg_kl_step(mi_net* net, mi_batch* b_corr, mi_batch* b_pred, mi_net* prior, mi_batch* b_prior, const float* coef_dev, int T,
                       const float* time_freqs, const float* traj_atom_types, const float* traj_frac, const float* traj_frac_mid,
                       const float* traj_lattices, const float* traj_lp_old, const int* t_host, const int* t_dev, const float* adv_dev,
                       float clip_range, const float* w_host, float loss_scale, float kl_coef, float* log_prob, float* kl_out,
                       float* grad_theta, float* stats, void* stream, void* aux_stream);

#ifdef __cplusplus
}
#endif

#endif
