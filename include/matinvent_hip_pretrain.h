/*
 * matinvent_hip_pretrain.h -- one micro-step of SUPERVISED denoising training (DiffCSPModule.training_step, diffusion.py:457-486;
 * pretrain.fit).  Same conventions as matinvent_hip.h (device pointers unless a name ends in `_host`, int32 indices, 0 or a
 * negative MI_E* code); a header of its own because the entry lists of the other headers are fixed.
 *
 * One network, one uniformly drawn time per crystal, and torch's F.mse_loss over ALL elements of the mini-batch: with e = pred - target,
 *   loss_lattice = sum_b sum_9 e^2 / (9 b_global),  loss_coord = sum_i sum_3 e^2 / (3 n_global),  loss_type = sum_i sum_100 e^2 / (100 n_global),
 *   loss = cl loss_lattice + cx loss_coord + ct loss_type,
 *   d (loss / accum_steps) / d (pl, px, pt) = 2 cl e / (9 b_global accum_steps),  2 cx e / (3 n_global accum_steps),  2 ct e / (100 n_global accum_steps).
 * Every atom of the mini-batch weighs the same (a 171-atom crystal weighs 171 times a 1-atom crystal): NOT the per-crystal means of
 * mi_ft_micro_step.  No reward, no anchor penalty, no second network.
 */
#ifndef MATINVENT_HIP_PRETRAIN_H
#define MATINVENT_HIP_PRETRAIN_H

#include "matinvent_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mi_pretrain_micro_step: enqueued end to end on `stream`, no host synchronisation --
 *   1. times:    b's times[c] = clamp(t_dev[c], 1, T) and the crystal's schedule row sched_table_dev[t] ([T + 1][4] = sqrt(alpha_bar),
 *                sqrt(1 - alpha_bar), sigma, sigmas_norm: the columns of mi_add_noise_per_crystal).  t_host [B] holds the same times on the
 *                host and is checked against 1..T BEFORE anything is enqueued (MI_EINVAL); the device clamps as well, so two copies that
 *                disagree give wrong numbers, never a read outside the table;
 *   2. the time embedding and the forward noising (draw ids 7-9 at call `noise_step`, indexed through the handle's node / graph offsets,
 *                or the injected rand_l [B][9] / rand_x [N][3] / rand_t [N][100]);
 *   3. the network's training forward;
 *   4. the loss of the header comment: the three gradient seeds and the per-crystal sums of squares;
 *   5. stats (4 floats, += ; or NULL):  [0] loss,  [1] loss_lattice,  [2] loss_coord,  [3] loss_type  -- fixed order, no atomics: the same
 *                bits every call;
 *   6. out_parts [B][3] or NULL: crystal b's sums of e^2 over its lattice, coordinate and type elements;
 *   7. the backward into grad_theta (+=).
 * grad_theta == NULL is the forward-only form (the validation loss): no tape is prepared and no backward runs; stats and out_parts are
 * those of the taped call up to the rounding of the inference forward.
 * b_global >= B and n_global >= N: the crystal and atom counts of the WHOLE mini-batch when the handle holds a shard of it.
 * B = 0: MI_OK, nothing is launched.  MI_EINVAL before anything is enqueued: a handle with a time map (mi_batch_set_time_map), with a
 * condition or a likelihood mask, with pending deferred weight gradients (mi_batch_wgrad_pending) or -- taped form -- an open
 * weight-gradient window; a time outside 1..T; counts below the handle's; accum_steps < 1. */
int mi_pretrain_micro_step(mi_net* net, mi_batch* b, const float* lengths, const float* angles, const float* frac0, const int* atom_types,
                           const float* time_freqs, const int* t_host, const int* t_dev, const float* sched_table_dev, int T, uint64_t seed,
                           uint32_t noise_step, const float* rand_l, const float* rand_x, const float* rand_t, float cost_lattice,
                           float cost_coord, float cost_type, int b_global, int n_global, int accum_steps, float* grad_theta, float* stats,
                           float* out_parts, void* stream);

#ifdef __cplusplus
}
#endif

#endif
