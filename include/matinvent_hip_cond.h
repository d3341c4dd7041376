/*
 * matinvent_hip_cond.h -- replacement conditioning of the reverse chain (RePaint, Lugmayr et al. 2022): a batch handle's
 * CONDITION names the part of the state that is known -- atom types, fractional coordinates per atom, the lattice per crystal -- and its
 * clean values.  Same conventions as matinvent_hip.h (device pointers unless a name ends in `_host`, int32 indices, 0 or a negative MI_E*
 * code); a header of its own because the entry lists of the other headers are fixed.
 *
 * Imposing the condition at noise level k overwrites the known elements with a forward-noised copy of their clean values
 * (DiffCSPModule.add_noise, diffusion.py:90-113), the unknown ones are neither read nor written nor drawn for:
 *   lattice      l = c0_k l0 + c1_k z                 c0_k = sqrt(abar_k), c1_k = sqrt(1 - abar_k)
 *   coordinates  x = (x0 + sigma_k z) mod 1
 *   atom types   a = c0_k onehot(type0) + c1_k z
 * At level 0 nothing is drawn and the table is not read: exactly l0, x0 mod 1 and a 1.0 / 0.0 one-hot row.
 * z is the counter-based Philox normal of the noise contract with the draw ids 21 (lattice), 22 (coordinates), 23 (types), the step field
 * = the level and the element index = (node_offset + atom) * width + column (graph_offset + crystal for the lattice): split batches and
 * shards draw the same numbers.  Separately rounded fp32 (no contraction), like the sampler's own updates.
 */
#ifndef MATINVENT_HIP_COND_H
#define MATINVENT_HIP_COND_H

#include "matinvent_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The condition of a batch handle of N atoms in B crystals.  Every pointer is HOST memory and is read by mi_batch_set_condition only.
 * A NULL mask means "none known"; the clean values of a part are needed only where its mask is nonzero (their pointer may be NULL when
 * the mask is NULL or all zero). */
typedef struct mi_condition {
    const int* known_types_host;    /* [N] nonzero: the atom's type is given */
    const int* known_coords_host;   /* [N] nonzero: the atom's three coordinates are given */
    const int* known_lattice_host;  /* [B] nonzero: the crystal's lattice is given */
    const int* types0_host;         /* [N] atomic numbers 1..100 */
    const float* frac0_host;        /* [N][3] */
    const float* lat0_host;         /* [B][9] */
} mi_condition;

/* mi_batch_set_condition: attach `cond` and the level table level_table_host[n][3] = (c0_k, c1_k, sigma_k), k = 0 .. n - 1 (n = T + 1 of
 * the chains that will run on the handle; on a strided view the view's tables, so the level is the step index there too), or clear the
 * condition with cond = NULL (the table is then ignored).  MI_EINVAL, and the handle keeps what it had: n < 2 or no table; a known type
 * outside 1..100; a nonzero mask entry whose clean values are missing.  Everything is copied to the device HERE, with blocking copies --
 * never inside a chain; call it while no work of this handle is in flight. */
int mi_batch_set_condition(mi_batch* b, const mi_condition* cond, const float* level_table_host, int n);

/* mi_condition_apply: impose the handle's condition on the state (atom_types [N][100], frac [N][3], lattices [B][9]) at noise level
 * `level` in 0 .. n - 1: one launch (none when nothing is known), one block per crystal.  MI_EINVAL: no condition on the handle, or a
 * level outside the table.
 *
 * mi_sampler_run with a condition on the handle imposes it (a) at level t_start, after the initial wrap and before traj[t_start] is
 * recorded, and (b) at level t - 1 after the predictor of every step t, the recorded t - 1 slices included.  The corrector is left alone.
 * A conditioned chain is therefore exactly: mi_condition_apply at t_start, then for every t one unconditioned step followed by
 * mi_condition_apply at t - 1.  The condition's draws always come from Philox keyed by the chain's seed (teacher-forced `noise` does not
 * cover them).  mi_sampler_run refuses with MI_EINVAL, before anything is enqueued: a condition together with CSP mode
 * (mi_sampler_set_keep), and a level table whose length is not the call's T + 1.  A handle without a condition makes exactly the launches
 * it made before this header existed. */
int mi_condition_apply(mi_batch* b, int level, uint64_t seed, float* atom_types, float* frac, float* lattices, void* stream);

#ifdef __cplusplus
}
#endif

#endif
