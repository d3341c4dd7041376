/*
 * matinvent_hip_scalar.h -- the PROPERTY PREDICTOR: the CSPNet trunk with a scalar head (the reference's CSPNet(pred_scalar=True),
 * models/diffcsp/cspnet.py:145-147, 281-284; predictor.py).  Same conventions as matinvent_hip.h (device pointers unless a name
 * ends in `_host`, int32 indices, 0 or a negative MI_E* code); a header of its own because the entry lists of the other headers are fixed.
 *
 * The head: gf[b] = mean over the crystal's atoms of the final node features (after the final LayerNorm when the net has one), and
 *   out[b][p] = bias[p] + sum_f gf[b][f] W[p][f],     W [P][H], bias [P], P >= 1 (P = 1: the reference's scalar_out).
 * W and bias are device pointers of the caller's: they are NOT parameters of mi_net (mi_net_num_params and every offset are those of a
 * net without the head).  A host that keeps one flat vector [trunk theta | W | bias] hands slices of it, and of its gradient, to the entries.
 *
 * Clean inputs (both entries, one launch): type rows are exact one-hot floats of atom_types (int, 1..100), coordinates frac0 wrapped to
 * [0, 1), the lattice matrix of (lengths, angles) by the forward noising's arithmetic, and the time embedding of times[b] (device, [B]) or,
 * times == NULL, of t_all for every crystal.
 *
 * Loss of the micro-step, with e = out - yhat over the PRESENT targets (have[b][p] != 0; the device never tests a target for NaN):
 *   loss = sum_p (1 / P) sum_{b: have} l(e_bp) / count_global[p],     l = e^2 (MI_SCALAR_LOSS_MSE) or |e| (MI_SCALAR_LOSS_L1),
 *   d (loss / accum_steps) / d out[b][p] = 2 e / (P count_global[p] accum_steps)   or   sign(e) / (P count_global[p] accum_steps).
 * A missing target contributes exactly 0.f to the seed and to every statistic.  No atomics; every sum has a fixed order (the head's dot
 * product a fixed function of H): the same bits every call.
 */
#ifndef MATINVENT_HIP_SCALAR_H
#define MATINVENT_HIP_SCALAR_H

#include "matinvent_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_SCALAR_LOSS_MSE 0
#define MI_SCALAR_LOSS_L1 1

/* mi_scalar_forward: the inference form -> out [B][P].  The trunk, the final LayerNorm and the graph mean run as in mi_cspnet_forward; the
 * type, coordinate and lattice heads are not computed.  Nothing is attached to the handle (its scratch of this entry is allocated on
 * first use); a pooled handle is accepted on its pool's stream.  Refusals: those of mi_scalar_micro_step that concern the handle and P. */
int mi_scalar_forward(mi_net* net, mi_batch* b, const float* lengths, const float* angles, const float* frac0, const int* atom_types,
                      const float* time_freqs, const int* times, int t_all, const float* W, const float* bias, int P, float* out, void* stream);

/* mi_scalar_micro_step: one training micro-step, enqueued end to end on `stream`, no host synchronisation --
 *   1. the clean inputs and the trunk's TRAINING forward, the graph mean and the head;
 *   2. the loss of the header comment against yhat [B][P] (normalised targets) under have [B][P]: the seeds and the crystals' terms;
 *   3. stats (1 + 3 P floats, += ; or NULL):  [0] loss,  then per property  [1 + 3 p] sum e^2,  [2 + 3 p] sum |e|,  [3 + 3 p] present targets;
 *   4. out [B][P] or NULL;
 *   5. the head's backward:  grad_bias[p] += sum_b d_out[b][p],  grad_W[p][f] += sum_b d_out[b][p] gf[b][f] (a fixed tree over b),
 *      dgf[b][f] = sum_p d_out[b][p] W[p][f];
 *   6. the trunk's backward into grad_theta (+=), seeded from dgf ALONE: d hf[i] = dgf[g(i)] / n_g.  The lattice_out.*, type_out.* and
 *      coord_out.* slices of grad_theta are left untouched.
 * grad_theta == NULL is the forward-only form (the validation loss): no tape is prepared, no backward runs, grad_W / grad_bias are not
 * read; stats and out are those of the taped call up to the rounding of the inference forward.
 * have_host / count_global_host hold the same values as have / count_global on the host: count_global[p] is the number of present
 * targets of property p over the WHOLE mini-batch when the handle holds a shard of it.
 * B = 0: MI_OK, nothing is launched.  MI_EINVAL before anything is enqueued: a handle with a time map, a condition, a likelihood mask or
 * guidance, with pending deferred weight gradients or -- taped form -- an open weight-gradient window; a net with a latent part
 * (mi_net_latent_dim > 0); P < 1; yhat without have; a have_host entry other than 0 / 1; a count_global_host entry below the handle's own
 * count of present targets; accum_steps < 1; an unknown loss_kind; grad_theta without grad_W and grad_bias. */
int mi_scalar_micro_step(mi_net* net, mi_batch* b, const float* lengths, const float* angles, const float* frac0, const int* atom_types,
                         const float* time_freqs, const int* times, int t_all, const float* W, const float* bias, int P, const float* yhat,
                         const int* have, const int* have_host, const int* count_global, const int* count_global_host, int accum_steps,
                         int loss_kind, float* grad_theta, float* grad_W, float* grad_bias, float* stats, float* out, void* stream);

/* Parity read of the last call on this handle (either entry): the pooled features gf [B][H] and -- after a micro-step with targets -- the
 * seeds d_out [B][P]; either pointer may be NULL.  P is the last call's (d_out is laid out for
 * it): MI_ESTATE when the handle has run no such call, or its last one was for another P. */
int mi_scalar_read(const mi_batch* b, int P, float* gf, float* d_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
