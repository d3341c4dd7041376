/*
 * matinvent_hip_traj.h -- trajectory extension of the C ABI (include/matinvent_hip.h): the log-probabilities of one recorded
 * reverse-diffusion step under the current weights, and their gradient with respect to the network's parameters.
 *
 * Replaces DiffCSPModule.forward_logprb (models/diffcsp/diffusion.py:158-227), the consumer of the trajectories that
 * sample_mdp (models/diffcsp/sample.py:249-309) records.  Same conventions as matinvent_hip.h (device pointers unless a name ends
 * in `_host`, fp32, int32 indices, row-major, `stream` = hipStream_t as void*, 0 or a negative MI_E* code); it is a header of
 * its own because the boundary header's entry count is fixed.
 */
#ifndef MATINVENT_HIP_TRAJ_H
#define MATINVENT_HIP_TRAJ_H

#include "matinvent_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mi_traj_logprob: re-evaluate one recorded step per crystal.  Crystal b sits at its own diffusion time t_dev[b] in 2..T (the
 * reference reads timesteps[0] for every crystal; both agree whenever the times are equal); anything else is MI_EINVAL (the
 * reference's formulas give inf / NaN at t = 1).  t_dev is read back to the host for that check (one synchronisation of `stream`).
 *   coef_dev [T+1][MI_NCOEF]  the per-step scalars (MI_C_*, the table mi_sampler_run takes, on the device)
 *   time_freqs                the time-embedding frequency table (mi_time_embedding)
 *   state at t:   atom_types [N,A], frac [N,3] (wrapped), frac_mid [N,3] (traj[t]['frac_coords_mid']), lattices [B,3,3]
 *   state at t-1: next_atom_types [N,A], next_frac [N,3], next_lattices [B,3,3]
 * Two network evaluations -- the corrector on (atom_types, frac, lattices) on batch handle b_corr, the predictor on
 * (atom_types, frac_mid, lattices) on b_pred: two distinct handles of `net` over the same atom counts -- then one kernel writes
 *   log_prob [3][B] = { log_prob_l, log_prob_t, log_prob_x } (diffusion.py:175-225; naive 21-image wrapped normal, per-crystal
 *   means in a fixed order: identical calls give identical bits)
 * and the corrector's raw predictions into pred_corr_l [B,3,3], pred_corr_x [N,3], pred_corr_t [N,A] (each may be NULL).
 * keep_tape = 1: both evaluations keep their activations (mi_cspnet_forward_train) and the kernel keeps the local derivatives, for
 * one mi_traj_logprob_backward; keep_tape = 0: inference evaluations, nothing kept. */
int mi_traj_logprob(mi_net* net, mi_batch* b_corr, mi_batch* b_pred, const int* t_dev, const float* coef_dev, int T,
                    const float* time_freqs, const float* atom_types, const float* frac, const float* frac_mid,
                    const float* lattices, const float* next_atom_types, const float* next_frac, const float* next_lattices,
                    float* log_prob, float* pred_corr_l, float* pred_corr_x, float* pred_corr_t, int keep_tape, void* stream);

/* mi_traj_logprob_backward: given g_logp [3][B] = dLoss/d(log_prob_l, log_prob_t, log_prob_x) and optional upstream gradients on
 * the returned corrector predictions (d_corr_l [B,3,3], d_corr_x [N,3], d_corr_t [N,A]; each may be NULL = zero), ACCUMULATES
 * dLoss/dtheta into grad_theta (`+=`, like mi_cspnet_backward): one kernel writes both evaluations' output gradients, then
 * mi_cspnet_backward runs on the predictor's and the corrector's tapes.  MI_ESTATE if the last call on (b_corr, b_pred) did not keep
 * its tape, or if either handle has been evaluated since (its tape was overwritten). */
int mi_traj_logprob_backward(mi_net* net, mi_batch* b_corr, mi_batch* b_pred, const float* g_logp, const float* d_corr_l,
                             const float* d_corr_x, const float* d_corr_t, float* grad_theta, void* stream);

#ifdef __cplusplus
}
#endif

#endif
