/*
 * matinvent_hip_guidance.h -- a property-conditioned DiffCSP prior and classifier-free guidance: the crystal embedding
 * [time | property], the supervised training micro-step with condition dropout, and the guided reverse step.  Same conventions as
 * matinvent_hip.h (device pointers unless a name ends in `_host`, int32 indices, 0 or a negative MI_E* code); a header of its own
 * because the entry lists of the other headers are fixed.
 *
 * A crystal carries P >= 1 scalar properties, normalised on the host: yhat [B][P] float32 with have [B][P] int32 (0: missing -- the
 * device never tests for NaN).  Row b of the embedding has TD = time_dim + Z columns, Z = 2 F P:
 *   [0, time_dim)                 the time embedding, time_embedding_kernel's arithmetic (through the handle's time map when it has one);
 *   time_dim + p 2F + k           sin(w_k y),      y = yhat[b][p] clamped to [-8, 8], w_k = prop_freqs[k] = (pi / 8) 2^k, k < F <= 12;
 *   time_dim + p 2F + F + k       cos(w_k y).
 * The NULL condition -- have = 0, a dropped crystal, or yhat == NULL -- is 2F columns of exactly 0.f: sin^2 + cos^2 = 1 for every
 * value, so no value can be taken for it.
 */
#ifndef MATINVENT_HIP_GUIDANCE_H
#define MATINVENT_HIP_GUIDANCE_H

#include "matinvent_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_GUIDANCE_MAX_FREQS 12
#define MI_GUIDANCE_CLAMP 8.0f

/* Record on `net` that the last Z = 2 F P columns of its embedding input (mi_net_config.time_dim = TD columns in all) are the property
 * part.  P = 0 clears it (Z = 0: the net of before).  MI_EINVAL unless P >= 0, 1 <= F <= 12 and TD - Z is a positive even number (the
 * time part is [sin | cos] halves; the products over K = TD ask TD % 4 == 0 and nothing more, which mi_net_create has checked). */
int mi_net_set_latent(mi_net* net, int P, int F);
/* Z of the net (0: none). */
int mi_net_latent_dim(const mi_net* net);

/* out [B][TD] = the embedding rows above, one thread per element.  times [B] or NULL (every crystal at t_all); `b` or NULL: a handle
 * whose time map the time part goes through (times / t_all are then step indices); nothing else of the handle is read.
 * yhat == NULL: every row null; otherwise have [B][P] is required.  drop [B] int32 or NULL: a non-zero entry makes the row null. */
int mi_crystal_embedding(const mi_net* net, const mi_batch* b, int B, const int* times, int t_all, const float* time_freqs,
                         const float* prop_freqs, const float* yhat, const int* have, const int* drop, float* out, void* stream);

/* drop [B] int32: crystal c is dropped (1) when the Philox uniform at (seed, call id `noise_step`, draw id 28, element graph_offset + c)
 * lies below p_uncond -- what mi_pretrain_micro_step_cond draws for a handle at that graph offset. */
int mi_guidance_drop_mask(uint64_t seed, uint32_t noise_step, int64_t graph_offset, int B, float p_uncond, int* drop, void* stream);

/* mi_pretrain_micro_step (matinvent_hip_pretrain.h) on a net with Z > 0: the same sequence with the embedding above in place of the
 * time embedding.  yhat / have as above (yhat == NULL: every crystal null); condition dropout: crystal c is null when the uniform of
 * mi_guidance_drop_mask at the handle's graph offset lies below p_uncond (0: no draw is made; data-parallel shards drop what the whole
 * mini-batch drops).  Takes a pooled handle; attaches nothing to the handle.  MI_EINVAL as mi_pretrain_micro_step, and for a net with
 * Z = 0, a missing prop_freqs, yhat without have, p_uncond outside [0, 1]. */
int mi_pretrain_micro_step_cond(mi_net* net, mi_batch* b, const float* lengths, const float* angles, const float* frac0, const int* atom_types,
                                const float* time_freqs, const int* t_host, const int* t_dev, const float* sched_table_dev, int T, uint64_t seed,
                                uint32_t noise_step, const float* rand_l, const float* rand_x, const float* rand_t, float cost_lattice,
                                float cost_coord, float cost_type, int b_global, int n_global, int accum_steps, float* grad_theta, float* stats,
                                float* out_parts, const float* prop_freqs, const float* yhat, const int* have, float p_uncond, void* stream);

/* Attach guidance to a classic handle: mi_sampler_run then evaluates the network under yhat_host / have_host [B][P] (copied; blocking
 * copies, no work of the handle may be in flight) and, with gamma != 0, a second time under the null condition on `partner` -- a handle
 * of the same atom counts and offsets with caches of its own -- and replaces every prediction by p_c + gamma (p_c - p_u) (the
 * corrector's coordinate head alone at the corrector stage).  gamma == 0: the conditional chain, partner unused (it may be NULL).
 * The frequency table (pi / 8) 2^k is built here.  MI_EINVAL: a pooled handle, a knn handle, partner == b, other atom counts or offsets,
 * P < 1, F outside 1..12, a non-finite gamma.  mi_sampler_run refuses (MI_EINVAL, before anything is enqueued) guidance together with
 * a record, a likelihood mask, a replacement condition, resampling, CSP mode, a net with Z = 0 or P / F other than the net's. */
int mi_batch_set_guidance(mi_batch* b, mi_batch* partner, const float* yhat_host, const int* have_host, int P, int F, float gamma);
int mi_batch_clear_guidance(mi_batch* b);

/* out = p_c + gamma (p_c - p_u), separately rounded (out may be p_c), over arrays of nl + nx + nt elements: the guided step's one launch,
 * whose three arrays -- lattice, coordinate and type predictions -- are the three consecutive segments of these. */
int mi_guidance_combine(const float* p_c, const float* p_u, float gamma, int64_t nl, int64_t nx, int64_t nt, float* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
