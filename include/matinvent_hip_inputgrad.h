/*
 * matinvent_hip_inputgrad.h -- CLASSIFIER GUIDANCE: the property predictor's INPUT gradient and the guided shift of a chain state
 * (classifier.py, predictor.py).  Same conventions as matinvent_hip.h (device pointers unless a name ends in `_host`, int32
 * indices, 0 or a negative MI_E* code); a header of its own because the entry lists of the other headers are fixed.
 *
 * The predictor (matinvent_hip_scalar.h) maps a chain state -- float type rows [N][100], coordinates [N][3], lattice matrices [B][9] --
 * and a time to out [B][P].  mi_scalar_input_grad hands out d(sum_p d_out[b][p] out[b][p]) / d(that state): the trunk's TRAINING forward,
 * the head, and the trunk's backward in its DATA-ONLY form -- no weight-gradient contraction, no gradient buffer -- carried down to the
 * inputs.  Dhariwal & Nichol's classifier guidance shifts the mean of a reverse step by scale * Sigma * grad log p(y | x_t): mi_guide_seed
 * forms the seed of log p(y | x_t) from the predictor's output, mi_guide_shift applies the shift.  Three entries.  None of them
 * synchronises with the host, none uses atomics, every sum has a fixed order: the same bits every call.
 */
#ifndef MATINVENT_HIP_INPUTGRAD_H
#define MATINVENT_HIP_INPUTGRAD_H

#include "matinvent_hip_steer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_GUIDE_MODE_MAX 0      /* d_out[b][p] = +1 */
#define MI_GUIDE_MODE_MIN 1      /* d_out[b][p] = -1 */
#define MI_GUIDE_MODE_TARGET 2   /* d_out[b][p] = -(out[b][p] - target_hat): the gradient of a unit-width Gaussian log-likelihood (the width lives in the scale) */

/* mi_scalar_input_grad: enqueued end to end on `stream` --
 *   1. mi_scalar_forward_state's inputs (the caller's arrays, read where they are and left unchanged) and time embedding (times [B] on
 *      the device or, times == NULL, t_all), with the trunk's TRAINING forward (the tape), the graph mean and the head -> out [B][P];
 *   2. dgf = d_out W, d hf[i] = dgf[g(i)] / n_g, and the trunk's backward in its data-only form down to
 *        g_frac  [N][3]     per layer l = L - 1 ... 0:  [dS | dC] = [Dm Wsin | Dp Wcos]  (Dm / Dp: the pair differences / sums of dZ1, Wsin / Wcos:
 *                           the layer's Fourier columns of edge_mlp.0.weight),  dDelta[p][d] += sum_k w_k (dS[p][d][k] cos(w_k Delta_pd) -
 *                           dC[p][d][k] sin(w_k Delta_pd)),  w_k = 2 pi k, with the forward's own argument arithmetic for Delta = (x_j - x_i) % 1
 *                           of pair (i < j);  then per atom, its pairs in ascending pair order:  g_frac[j] += dDelta[p],  g_frac[i] -= dDelta[p].
 *                           A crystal of one atom has no pair: its row is exactly 0;
 *        g_lat   [B][9]     M[q] = sum_l sum_c dG_l[b][c] W_l[c][2H + q] (l = L - 1 ... 0, c in a fixed tree), then (M + M^T) L: the chain rule
 *                           of the Gram matrix L L^T;
 *        g_types [N][100]   dXa node_embedding.weight (c ascending); NULL: not computed.
 * Crystals are independent: row b of the results is d(sum_p d_out[b][p] out[b][p]) / d(inputs of crystal b).
 * MI_EINVAL with a named message before anything is enqueued: a knn-style handle; a pooled handle; a handle with a time map, a condition,
 * a likelihood mask or guidance, with pending deferred weight gradients or an open weight-gradient window; a net with a latent part; pair
 * mode switched off or hidden_dim % 4 != 0; P < 1; a null argument.  B = 0: MI_OK, nothing is launched. */
int mi_scalar_input_grad(mi_net* net, mi_batch* b, const float* atom_types, const float* frac, const float* lattices, const float* time_freqs,
                         const int* times, int t_all, const float* W, const float* bias, int P, const float* d_out, float* out, float* g_types,
                         float* g_frac, float* g_lat, void* stream);

/* mi_guide_seed: d_out [B][P] from out [B][P] -- column p by `mode` (above), every other column 0; a row whose out[b][p] is not finite is
 * all zeros.  One launch.  MI_EINVAL: B < 0, P < 1, p outside 0 .. P - 1, an unknown mode, a non-finite target_hat in TARGET mode. */
int mi_guide_seed(const float* out, int B, int P, int p, int mode, float target_hat, float* d_out, void* stream);

/* mi_guide_shift: state += a g in place, one workgroup per crystal --
 *   lattices[b][q] += clamp(a_l g_lat[b][q]),  frac[i][d] = pymod1(frac[i][d] + clamp(a_x g_frac[i][d])),  and, g_types != NULL,
 *   atom_types[i][k] += clamp(a_t g_types[i][k]);   clamp(v) = min(max(v, -max_shift), max_shift) when max_shift > 0, v otherwise.
 * A crystal ANY of whose gradient elements (of the arrays given) is not finite is left unchanged bit for bit -- its coordinates are not
 * even re-wrapped.  csrc/guide_shift.h holds the arithmetic (host and device).  MI_EINVAL: a non-finite coefficient or max_shift, a null
 * argument, a pooled handle on another stream than its pool's. */
int mi_guide_shift(mi_batch* b, float* atom_types, float* frac, float* lattices, const float* g_types, const float* g_frac, const float* g_lat,
                   float a_t, float a_x, float a_l, float max_shift, void* stream);

#ifdef __cplusplus
}
#endif

#endif
