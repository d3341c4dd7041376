/*
 * matinvent_hip_symc.h -- symmetry-constrained sampling: a batch handle's SYMMETRY CONSTRAINT names, per crystal, a group of
 * operations and the orbits of the atoms under it; imposing it projects a state of the reverse chain -- coordinates, cell and type rows --
 * onto the states that carry that group exactly, to float32 rounding.  Same conventions as matinvent_hip.h (device pointers unless a name
 * ends in `_host`, int32 indices, 0 or a negative MI_E* code); a header of its own because the entry lists of the other headers are fixed.
 * All arithmetic is float64 or exact integers; matinvent_amd/csrc/sym_constraint.h holds every formula.
 *
 * Definition (one 256-thread workgroup per crystal), in the basis of the state's own cell, where an operation is g_k(f) = f W_k^-1 + t_k
 * and the rows of the cell L are its vectors.  For a crystal with K > 1 operations, R distinct rotation parts and n atoms:
 *   coordinates  x_j <- wrap(x_r Q_j + d_j), r = rep[j], for every atom (representatives too): float64 from the float32 coordinates of the
 *                representative, as they were before the call, rounded once to float32 in [0, 1) (a float that rounds to 1 is 0)
 *   cell         G = L L^T in float64; Gbar = (sum over the R distinct rotation parts of W G W^T) / R, the sum through the fixed tree over
 *                256 slots (slot i < s takes slot i + s, s = 128 .. 1; zeros above R); the new cell is the lower Cholesky factor of Gbar
 *                (a along x, b in the xy plane), rounded once to float32.  A non-finite Gbar or a pivot that is not positive: the cell
 *                keeps every bit and the crystal's failure counter goes up by one.
 *   type rows    row_j <- row_r (100 floats) for every atom that is not its own representative
 * A crystal with K = 1 keeps every bit of all three parts.
 */
#ifndef MATINVENT_HIP_SYMC_H
#define MATINVENT_HIP_SYMC_H

#include "matinvent_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_SYMC_MAX_ATOMS 256
#define MI_SYMC_MAX_OPS 192

/* The constraint of a batch handle of N atoms in B crystals.  Every pointer is HOST memory and is read by mi_batch_set_symmetry only. */
typedef struct mi_symmetry_constraint {
    const int* op_off_host;        /* [B + 1] first operation of each crystal; K_b = op_off[b + 1] - op_off[b] in 1 .. 192 */
    const int* rot_host;           /* [op_off[B]][9] the rotation parts W_k */
    const int* distinct_off_host;  /* [B + 1] first entry of each crystal in distinct_host */
    const int* distinct_host;      /* [distinct_off[B]] operations (indices inside the crystal) whose rotation parts are the distinct ones */
    const int* rep_host;           /* [N] the orbit representative of each atom, an index inside the crystal */
    const double* Q_host;          /* [N][9] */
    const double* d_host;          /* [N][3] */
} mi_symmetry_constraint;

/* mi_batch_set_symmetry: attach the constraint, or clear it with c = NULL.  MI_EINVAL, and the handle keeps what it had: a null array;
 * offsets that do not start at 0 or decrease; K outside 1 .. 192; a crystal of more than 256 atoms with K > 1; det W != +-1; a distinct
 * list that is empty, leaves its crystal, names a rotation part twice or misses one; a representative outside its crystal or one that is
 * not its own representative; a non-finite Q / d.  Everything is copied to the device HERE, with blocking copies -- never inside a chain;
 * call it while no work of this handle is in flight.  The failure counters are cleared. */
int mi_batch_set_symmetry(mi_batch* b, const mi_symmetry_constraint* c);

/* mi_symmetry_apply: impose the handle's constraint on the state (atom_types [N][100], 16-byte aligned; frac [N][3]; lattices [B][9]), in
 * place: one launch, none when every crystal has K = 1.  MI_EINVAL: no constraint on the handle.
 *
 * mi_sampler_run with a constraint on the handle imposes it (a) at t_start, after the initial wrap and after any condition, and (b) after
 * the predictor of every step, after the condition's imposition.  The corrector is left alone.  A constrained chain is therefore exactly:
 * mi_symmetry_apply, then for every t one unconstrained step followed by mi_symmetry_apply.  mi_sampler_run refuses with MI_EINVAL,
 * before anything is enqueued, a constraint together with: a record, teacher-forced noise, CSP mode, resampling jumps, guidance (a
 * projected state has no likelihood under the recorded proposal), or a condition that knows any coordinate or lattice (a condition on
 * atom types alone is allowed).  A handle without a constraint makes exactly the launches it made before this header existed. */
int mi_symmetry_apply(mi_batch* b, float* atom_types, float* frac, float* lattices, void* stream);

/* mi_symmetry_failures: the per-crystal count of cell projections skipped since the last call, into out_host [B], and cleared.  Blocking
 * copies: call it while no work of this handle is in flight. */
int mi_symmetry_failures(mi_batch* b, int* out_host);

#ifdef __cplusplus
}
#endif

#endif
