/*
 * matinvent_hip_resample.h -- resampling jumps for the conditioned reverse chain (RePaint's "time travel", Lugmayr et al. 2022).
 * Replacement conditioning (matinvent_hip_cond.h) overwrites the known part after every reverse step with a forward-noised copy drawn
 * independently of what the chain generated; the jumps give the generated part several passes at adapting to it: at every jump-off level
 * the whole state is re-noised j levels forward and denoised again, r visits in all.  Same conventions as matinvent_hip.h (device
 * pointers unless a name ends in `_host`, 0 or a negative MI_E* code); a header of its own because the entry lists of the other headers
 * are fixed.
 *
 * The schedule.  Levels are the chain's own: T .. 0, or step indices on a strided view.  A chain with resampling (r, j), r >= 1, j >= 1,
 * started at t_start:
 *     left[L] = r - 1 for every jump-off level L = 1, 1 + j, 1 + 2 j, ... with L + j <= t_start
 *     t = t_start
 *     while t > 0:
 *         reverse step t -> t - 1 (corrector, predictor, imposition at t - 1)
 *         t -= 1
 *         if left[t] > 0: left[t] -= 1; forward jump t -> t + j; t += j
 * The chain never jumps from level 0: the step 1 -> 0 runs once and the known part is exact at the end.  r = 1 is the plain chain.
 *
 * The forward jump from level a to b = a + j is one draw applied to EVERY element of the state, known or not (a known element imposed at
 * a and jumped to b is distributed like an imposition at b, so no imposition follows a jump):
 *   lattice      l <- c0 l + c1 z                     c0 = sqrt(abar_b / abar_a), c1 = sqrt(1 - abar_b / abar_a)
 *   atom types   a <- c0 a + c1 z
 *   coordinates  x <- (x + s z) mod 1                 s = sqrt(sigma_b^2 - sigma_a^2); wrapped twice, the state stays in [0, 1)
 * Separately rounded fp32 (no contraction).  Row a of the jump table [T + 1][3] holds (c0, c1, s) of a -> a + j; rows with a + j > T are
 * zero.  The caller computes it in float64 and rounds it to float32 (in float32 1 - c0^2 cancels at early levels).
 *
 * Noise contract.  z is the Philox normal with the draw ids 24 (lattice), 25 (coordinates), 26 (types), the step field = the level
 * jumped TO and the element index of every other draw ((node_offset + atom) * width + column; graph_offset + crystal for the lattice).
 * Every repetition has a seed of its own: seed_0 = seed, and for v >= 1 seed_v = words 0 (low) and 1 (high) of the Philox block with
 * counter (0, 0, 27, v) under the key `seed`.  The v-th execution (0-based) of the transition t -> t - 1 and the imposition at t - 1 that
 * follows it use seed_v; the v-th jump (1-based) off a level uses seed_v; the initial draw and the imposition at t_start use seed.  No
 * (seed_v, level, draw id) occurs twice in a chain, and with r = 1 every draw is keyed by `seed` as before.
 */
#ifndef MATINVENT_HIP_RESAMPLE_H
#define MATINVENT_HIP_RESAMPLE_H

#include "matinvent_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mi_batch_set_resampling: attach (r, j) and jump_table_host[n][3] (n = T + 1 of the chains that will run on the handle), or clear with
 * jump_table_host = NULL (n, r, j are then ignored).  MI_EINVAL, and the handle keeps what it had: n < 2, a non-finite table entry,
 * r < 1, j < 1 or j >= n.  The table is copied to the device HERE, with a blocking copy -- never inside a chain; call it while no work of
 * this handle is in flight.
 *
 * mi_sampler_run on a handle with resampling and r > 1 walks the schedule above: the same launches per reverse step as the plain
 * conditioned chain, one more per jump, no host round trip.  It refuses with MI_EINVAL, before anything is enqueued: no condition on the
 * handle; a record (`rec`); teacher-forced `noise`; a likelihood mask; t_stop != 0; a table whose length is not the call's T + 1; no
 * jump-off level at all (1 + j > t_start).  With r = 1, or without resampling, the chain makes exactly the launches it made before. */
int mi_batch_set_resampling(mi_batch* b, const float* jump_table_host, int n, int r, int j);

/* mi_resample_jump: the forward jump from_level -> from_level + j of the state (atom_types [N][100], frac [N][3], lattices [B][9]), in
 * place: one launch, one block per crystal.  MI_EINVAL: no resampling on the handle, or from_level < 0 or from_level + j outside the
 * table. */
int mi_resample_jump(mi_batch* b, int from_level, uint64_t seed, float* atom_types, float* frac, float* lattices, void* stream);

/* mi_resample_schedule (host only): the levels a chain with (t_start, r, j) visits, t_start first and 0 last.  Returns their number
 * (reverse steps + jumps + 1) and writes the first min(cap, number) of them to levels_out_host (which may be NULL when cap = 0).
 * MI_EINVAL: t_start < 0, r < 1, j < 1, cap < 0. */
int64_t mi_resample_schedule(int t_start, int r, int j, int* levels_out_host, int64_t cap);

/* mi_resample_visit_seed (host only): seed_v of the contract above; v = 0 returns `seed`. */
uint64_t mi_resample_visit_seed(uint64_t seed, uint32_t v);

#ifdef __cplusplus
}
#endif

#endif
