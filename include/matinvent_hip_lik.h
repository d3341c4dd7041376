/*
 * matinvent_hip_lik.h -- the trajectory likelihood of a CONDITIONED reverse chain: a batch handle's LIKELIHOOD MASK names
 * the elements that replacement conditioning (matinvent_hip_cond.h) overwrites after every step -- atom types and coordinates per atom,
 * the lattice per crystal.  Same conventions as matinvent_hip.h (0 or a negative MI_E* code); a header of its own because the entry
 * lists of the other headers are fixed.
 *
 * In a conditioned step s_t -> s_{t-1} the corrector moves every coordinate (its outcome x_mid is recorded), the predictor proposes
 * s'_{t-1}, and the imposition overwrites the known elements of s' with a draw that depends neither on the weights nor on s'.  Every
 * predictor transition factorises per element, so marginalising the discarded known part of s' gives
 *   log p(x_mid, s_{t-1} | s_t) = corrector term over ALL atoms + predictor terms over the FREE elements + a weight-independent constant.
 * With a mask on the handle, per crystal of n atoms:
 *   log_prob_l  0 where known_lattice, else unchanged
 *   log_prob_t  the sum over atoms with known_types == 0 of the per-atom mean over the 100 logits, divided by n (NOT by the free count)
 *   log_prob_x  the corrector mean over all 3 n coordinates + the predictor sum over atoms with known_coords == 0, over 3 and over n
 * The local derivatives of a taped call (dl, dt, dx_pred) are exactly 0.f at masked elements and unchanged elsewhere, dx_corr is
 * unchanged everywhere.  The KL anchor drops the same elements of the predictor's lattice, type and coordinate terms and derivatives
 * with the same divisors; its corrector coordinate term stays over all atoms.  The divisors being kept, every free element contributes
 * the bits it contributes without a mask, and an all-zero mask gives the bits of a handle without one.
 *
 * Who reads the mask:
 *   mi_traj_logprob, mi_traj_pg_step, mi_traj_pg_kl_step  take the masked kernels when the PREDICTOR handle carries a mask.  Both handles
 *       of the pair (and the prior's handle of the KL entry) must carry the same mask or none: MI_EINVAL before anything is enqueued.
 *   mi_sampler_run  a recording chain on a handle that carries BOTH a condition and a mask records the masked log_prob_l / t / x.  The
 *       states, the corrector's record and the launches of every other handle are those of before.
 */
#ifndef MATINVENT_HIP_LIK_H
#define MATINVENT_HIP_LIK_H

#include "matinvent_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mi_batch_set_likelihood_mask: attach the masks known_types [N], known_coords [N], known_lattice [B] (HOST memory, int32, each entry 0
 * or 1) to a batch handle of N atoms in B crystals, or clear the mask with three NULLs.  A NULL among non-NULL pointers means "none
 * known" for that part.  Separate from mi_batch_set_condition: the mask needs no clean values and no level table.  MI_EINVAL, and the
 * handle keeps what it had: an entry other than 0 or 1.  Everything is copied to the device HERE, with blocking copies -- never inside
 * a chain or a micro-step; call it while no work of this handle is in flight. */
int mi_batch_set_likelihood_mask(mi_batch* b, const int* known_types, const int* known_coords, const int* known_lattice);

/* mi_batch_has_likelihood_mask: 1 when the handle carries a mask (an all-zero one included), 0 when not; MI_EINVAL for a NULL handle. */
int mi_batch_has_likelihood_mask(const mi_batch* b);

/* mi_traj_read_derivatives: copy the local derivatives that the last TAPED mi_traj_logprob / mi_traj_pg_step / mi_traj_pg_kl_step left on
 * a batch handle -- d log_prob / d(network output) per element, before any upstream gradient -- into dl [B][9], dx [N][3], dt [N][100]
 * (device memory; each may be NULL: not copied), enqueued on `stream`.  The predictor handle of the call holds dl, dx_pred and dt, the
 * corrector handle dx_corr (its dl / dt are not written by a call).  MI_ESTATE: no taped call has used the handle yet.  For tests of the
 * masked forms: the derivatives are exactly 0.f at masked elements. */
int mi_traj_read_derivatives(const mi_batch* b, float* dl, float* dx, float* dt, void* stream);

#ifdef __cplusplus
}
#endif

#endif
