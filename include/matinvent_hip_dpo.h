/*
 * matinvent_hip_dpo.h -- the preference (Diffusion-DPO) fine-tune micro-step on ranked pairs of FINAL crystals (preference.dpo_step;
 * DESIGN 34).  Same conventions as matinvent_hip.h (device pointers unless a name ends in `_host`, int32 indices, 0 or a negative MI_E*
 * code); a header of its own because the entry lists of the other headers are fixed.
 *
 * With the per-crystal denoising loss of mi_ft_micro_step,
 *   L_b(p) = cl mean9((pl - rl)^2) + cx mean_i mean3((px - tx)^2) + ct mean_i mean100((pt - rt)^2),
 * and both networks evaluated on the same noised input at the same time:
 *   d_b = L_b(agent) - L_b(prior)                 accumulated element-wise as (pa - pp)(pa + pp - 2 target): never a difference of two sums
 *   pair p = (w, l):  m_p = d_w - d_l,  u_p = beta m_p,  loss_p = softplus(u_p) = -log sigmoid(-u_p),  g_p = sigmoid(u_p)
 *   total = inv_denom sum_p loss_p,               inv_denom = 1 / (p_global accum_steps)
 *   c_b = inv_denom beta (sum_{p: w_p = b} g_p - sum_{p: l_p = b} g_p)
 *   d total / d (pl, px, pt) = c_b cl 2 (pl - rl) / 9,  c_b cx 2 (px - tx) / (3 n_b),  c_b ct 2 (pt - rt) / (100 n_b).
 * softplus and sigmoid are evaluated in overflow-free forms (max(u, 0) + log1p(exp(-|u|)), the two-branch sigmoid): finite for any finite u.
 */
#ifndef MATINVENT_HIP_DPO_H
#define MATINVENT_HIP_DPO_H

#include "matinvent_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mi_batch_set_pairs: attach the n_pairs >= 1 pairs (winners_host[p], losers_host[p]) of crystal indices of this handle, or clear them with
 * n_pairs = 0 (the arrays may then be NULL).  Every index must lie in [0, B) and a pair's two crystals must differ; n_pairs < 0, a NULL array
 * or a bad pair give MI_EINVAL and the handle keeps what it had.  A crystal may sit in any number of pairs, none included.  The arrays are
 * copied to the device HERE, with blocking copies; set them while no work of this handle is in flight. */
int mi_batch_set_pairs(mi_batch* b, const int* winners_host, const int* losers_host, int n_pairs);

/* The number of pairs the handle carries (0: none; NULL handle: 0). */
int mi_batch_num_pairs(const mi_batch* b);

/* mi_dpo_micro_step: one timestep of the preference fine-tune in one call -- the sequence of mi_ft_micro_step (time fill and embedding,
 * the forward noising with draw ids 7-9 at call `noise_step` or the injected rand_l / rand_x / rand_t, the agent's training forward, the
 * frozen prior's forward, forked onto aux_stream when given, the backward into grad_theta (+=)) with the loss stage of the header comment
 * over the pairs of `ab` (MI_ESTATE when it carries none).  p_global: the pair count the loss is normalised by (>= the handle's).
 *   stats (3 floats, += ; or NULL):  [0] sum_p loss_p / p_global,  [1] #{p : m_p < 0},  [2] sum_p (-m_p)
 *   out_delta [B] or NULL: d_b;   out_margin [n_pairs] or NULL: m_p.
 * A crystal in no pair gets gradient seeds that are exactly zero.  No atomics: the same bits run to run. */
int mi_dpo_micro_step(mi_net* agent, mi_batch* ab, mi_net* prior, mi_batch* pb, const float* lengths, const float* angles,
                      const float* frac0, const int* atom_types, const float* time_freqs, int t, float c0, float c1, float sigma_t,
                      float sigma_norm, uint64_t seed, uint32_t noise_step, const float* rand_l, const float* rand_x, const float* rand_t,
                      float cost_lattice, float cost_coord, float cost_type, float beta, int p_global, int accum_steps, float* grad_theta,
                      float* stats, float* out_delta, float* out_margin, void* stream, void* aux_stream);

#ifdef __cplusplus
}
#endif

#endif
