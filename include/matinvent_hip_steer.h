/*
 * matinvent_hip_steer.h -- PREDICTOR-STEERED SAMPLING (Feynman-Kac steering / sequential Monte Carlo with twisted particle resampling;
 * steering.py, predictor.py).  Same conventions as matinvent_hip.h (device pointers unless a name ends in `_host`, int32
 * indices, 0 or a negative MI_E* code); a header of its own because the entry lists of the other headers are fixed.
 *
 * A reverse chain runs K particles (replicas) per crystal.  At chosen noise levels a noise-aware property predictor scores every
 * particle's noisy state, and the particles of each group are resampled in proportion to exp(lambda (u - u_prev)): with these difference
 * potentials the weights telescope to exp(lambda u(x_0)), and the particle system targets p_prior(x_0) exp(lambda u(x_0)).  Three entries:
 *   mi_scalar_micro_step_noised   trains the predictor on forward-noised inputs at a drawn time per crystal;
 *   mi_scalar_forward_state       evaluates it on a chain STATE (float type rows, coordinates, lattice matrices);
 *   mi_steer_resample             weights, effective sample size, ancestors and the ragged gather of the state, on the device.
 * None of them synchronises with the host, none uses atomics, every sum has a fixed order: the same bits every call.
 */
#ifndef MATINVENT_HIP_STEER_H
#define MATINVENT_HIP_STEER_H

#include "matinvent_hip_scalar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_STEER_MODE_MAX 0      /* u = +out[k][p] */
#define MI_STEER_MODE_MIN 1      /* u = -out[k][p] */
#define MI_STEER_MODE_TARGET 2   /* u = -|out[k][p] - target_hat| */
#define MI_STEER_MAX_PARTICLES 256
#define MI_STEER_DRAW 29         /* the Philox draw id of the resampling uniform */
#define MI_STEER_NSTATS 3

/* mi_scalar_micro_step_noised: mi_scalar_micro_step on FORWARD-NOISED inputs, enqueued end to end on `stream` --
 *   1. times[c] = clamp(t_dev[c], 0, T) and the crystal's schedule row sched_table_dev[times[c]] = {sqrt(alpha_bar), sqrt(1 - alpha_bar),
 *      sigma, sigmas_norm} (a [T + 1][4] device table; row 0 is the clean row (1, 0, 0, .): at time 0 the inputs are mi_scalar_micro_step's,
 *      bit for bit in the type rows and the coordinates), and the time-embedding row of times[c];
 *   2. the forward noising of mi_add_noise_per_crystal: draws 7 / 8 / 9 at `noise_step`, indexed through the handle's node / graph
 *      offsets, or the injected rand_l [B][9] / rand_x [N][3] / rand_t [N][100] (each may be NULL on its own);
 *   3. mi_scalar_micro_step's steps 1 (from the trunk's forward) to 6 on those inputs: head, loss, stats (+=), out, the head's backward,
 *      the trunk's backward into grad_theta (+=), the three diffusion heads' slices untouched.
 * grad_theta == NULL is the forward-only (validation) form.  t_host holds t_dev's values on the host: a time outside 0..T is MI_EINVAL
 * before anything is enqueued (the device clamps as well, so that a stray value never reads outside the table).  The other refusals are
 * mi_scalar_micro_step's. */
int mi_scalar_micro_step_noised(mi_net* net, mi_batch* b, const float* lengths, const float* angles, const float* frac0, const int* atom_types,
                                const float* time_freqs, const int* t_host, const int* t_dev, const float* sched_table_dev, int T, uint64_t seed,
                                uint32_t noise_step, const float* rand_l, const float* rand_x, const float* rand_t, const float* W, const float* bias,
                                int P, const float* yhat, const int* have, const int* have_host, const int* count_global,
                                const int* count_global_host, int accum_steps, int loss_kind, float* grad_theta, float* grad_W, float* grad_bias,
                                float* stats, float* out, void* stream);

/* mi_scalar_forward_state: the inference form on a chain state -> out [B][P].  atom_types [N][100] float rows (whatever the chain holds:
 * noisy logits, not one-hot rows), frac [N][3], lattices [B][9] are read as given and left unchanged; the time embedding is that of
 * times[b] (device, [B]) or, times == NULL, of t_all.  `b` is a handle of the PREDICTOR's net with the chain's atom counts and offsets: the
 * chain's own handle and what it caches are never touched.  The trunk runs as in mi_scalar_forward (net_forward, trunk only), then the
 * head.  Refusals: mi_scalar_forward's. */
int mi_scalar_forward_state(mi_net* net, mi_batch* b, const float* atom_types, const float* frac, const float* lattices, const float* time_freqs,
                            const int* times, int t_all, const float* W, const float* bias, int P, float* out, void* stream);

/* mi_steer_resample: one resampling event of the particle system.  The handle's B crystals are G = B / K groups of K consecutive
 * replicas.  Two launches.
 *
 * PLAN (one workgroup per group; csrc/steer_plan.h holds its text and fixes every order of summation):
 *   u_k    = +out[k][p] (MI_STEER_MODE_MAX), -out[k][p] (MIN), -|out[k][p] - target_hat| (TARGET)        out [B][P], 0 <= p < P
 *   lw_k   = logw[k] + lambda (u_k - u_prev[k]);  a particle whose score is not finite has weight 0 (lw_k = -inf), and so has one whose
 *            lw_k is NaN (its previous score was not finite and it has not been resampled since)
 *   w_k    = exp(lw_k - max_k lw_k),   ESS = (sum w)^2 / sum w^2
 *   the group resamples when ess_frac < 0 (always) or ESS < ess_frac K.  Resampling is SYSTEMATIC from one uniform U per group: Philox
 *   draw MI_STEER_DRAW under `seed`, step field `level`, element index = the global index (graph offset included) of the group's first
 *   crystal -- mi_philox_fill(seed, level, 29, that index, 1, uniform = 1) is the same number.  Offspring j takes the smallest k whose
 *   cumulative sum w_0 + ... + w_k exceeds (U + j) / K * sum w.  A group whose weights are all bit-equal gets the identity by
 *   construction.  After a resampling u_prev[k] = u_{a_k} and logw[k] = 0; otherwise u_prev[k] = u_k and logw[k] = lw_k.
 *   A group with no particle of finite weight keeps the identity, u_prev and logw as they were, and is counted in stats[2].
 *   ancestors [B] (int): the crystal index inside the handle (0 .. B - 1) whose state crystal c receives; always inside c's group.
 * A first event starts from u_prev = 0 and logw = 0 (the caller's zeros).
 *
 * GATHER (one workgroup per crystal): dst rows of crystal c = src rows of crystal ancestors[c] -- type rows [n][100], coordinate rows
 * [n][3], the lattice [9]; 16-byte accesses for the type rows when both arrays are 16-byte aligned.  Nothing outside a crystal's rows is
 * read or written; src is unchanged.
 *
 * stats (MI_STEER_NSTATS floats, += ; or NULL): [0] groups that resampled, [1] the sum of the groups' ESS, [2] groups without a particle of
 * finite weight -- summed over the groups in a fixed order by one workgroup of the second launch.
 *
 * MI_EINVAL from the handle's host-side counts, before anything is enqueued: K < 1 or K > MI_STEER_MAX_PARTICLES; B % K != 0; a group
 * whose members differ in atom count; P < 1 or p outside 0 .. P - 1; an unknown mode; a non-finite lambda, ess_frac or (TARGET)
 * target_hat; a dst array overlapping its src array; a null argument.  B = 0: MI_OK, nothing is launched. */
int mi_steer_resample(mi_batch* b, int K, const float* out, int P, int p, int mode, float target_hat, float lambda, float ess_frac, uint64_t seed,
                      uint32_t level, float* u_prev, float* logw, const float* src_types, const float* src_frac, const float* src_lat,
                      float* dst_types, float* dst_frac, float* dst_lat, int* ancestors, float* stats, void* stream);

#ifdef __cplusplus
}
#endif

#endif
