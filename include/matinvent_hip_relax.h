/*
 * matinvent_hip_relax.h -- BATCHED STRUCTURE RELAXATION on a learned energy: FIRE on the device (relax.py, predictor.py).
 * Same conventions as matinvent_hip.h (device pointers unless a name ends in `_host`, int32 indices, 0 or a negative MI_E* code); a header
 * of its own because the entry lists of the other headers are fixed.
 *
 * The property predictor (matinvent_hip_scalar.h) maps a state -- float type rows [N][100], coordinates [N][3], lattice matrices [B][9] --
 * to out [B][P]; column p is read as an energy, and mi_scalar_input_grad (matinvent_hip_inputgrad.h) hands out its gradient with respect
 * to the coordinates and the lattice.  Lattice rows are cell vectors and cart = frac L, so the forces are
 *     F_i = -s_b g_frac[i] L^-T,       and with relax_cell three more rows   F_L = -s_b g_lat / c_b,
 *     s_b = scale (x n_b when per_atom),   c_b = cell_factor (<= 0: the atom count n_b),
 * and one step of FIRE (Bitzek et al. 2006, in the form of ASE's optimizer, whose constants are the defaults of relax.py) moves every
 * crystal that is still ACTIVE.  A crystal of n atoms has R = n (+ 3) rows of three degrees of freedom; every sum over them is one fixed
 * tree that is a function of R alone (csrc/relax_fire.h holds the arithmetic, host and device).  Three entries.  None of them synchronises
 * with the host, none uses atomics, every sum has a fixed order: the same bits every call.
 */
#ifndef MATINVENT_HIP_RELAX_H
#define MATINVENT_HIP_RELAX_H

#include "matinvent_hip_inputgrad.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_RELAX_ACTIVE 0
#define MI_RELAX_CONVERGED 1   /* max over the rows of |F row| < fmax, decided before any move */
#define MI_RELAX_FAILED 2      /* a non-finite gradient, output or lattice element, or |det L| < det_min */
#define MI_RELAX_EXHAUSTED 3   /* still ACTIVE when mi_relax_run(finish = 1) ended */

/* the per-crystal state: fstate [B][MI_RELAX_NF] floats, istate [B][MI_RELAX_NI] ints */
#define MI_RELAX_NF 6          /* dt, alpha, first energy, last energy, last max |F row|, last |dr| (before the clamp); energies are out[b][p], normalised */
#define MI_RELAX_NI 3          /* status, positive-power count, steps taken */
#define MI_RELAX_MAX_ROWS 1500 /* n + 3 of the handle's largest crystal: the workgroup's LDS holds 10 floats per row */

typedef struct {
    float dt, dt_max, maxstep, f_inc, f_dec, a_start, f_a, fmax;   /* all finite and > 0 */
    float scale;         /* std[p] of the property's normaliser, > 0: fmax is in the property's raw unit per Angstrom */
    float cell_factor;   /* c_b; <= 0: the crystal's atom count */
    float det_min;       /* > 0 */
    int n_min;           /* >= 0 */
    int relax_cell;      /* 0: the lattice and vel_l are never written, and the cell rows are absent from every sum */
    int per_atom;        /* 1: column p is an energy per atom */
} mi_relax_params;

/* mi_relax_init: vel_x [N][3] = 0, vel_l [B][9] = 0, fstate = (dt, a_start, 0, 0, 0, 0), istate = (ACTIVE, 0, 0) and the constant seed
 * d_out [B][P] (+1 in column p, 0 elsewhere).  One launch.  MI_EINVAL: a null handle or argument, a bad parameter (below), p outside 0 .. P - 1. */
int mi_relax_init(mi_batch* b, const mi_relax_params* params_host, int P, int p, float* vel_x, float* vel_l, float* fstate, int* istate,
                  float* d_out, void* stream);

/* mi_relax_step: one FIRE step of every crystal from given g_frac [N][3], g_lat [B][9] and out [B][P] -- one launch, one workgroup per crystal.
 * A crystal that is not ACTIVE keeps every bit of its state: its coordinates are not even re-wrapped.  Of an ACTIVE crystal, in this order:
 *   FAILED     a non-finite element of its g_frac, g_lat, out[b][p] or lattice, or |det L| < det_min: the status alone is written;
 *   the first energy (at step 0), the last energy and the last max |F row| are recorded;
 *   CONVERGED  max over the rows of |F row| < fmax: nothing else is written;
 *   the step   P = F.v;  P > 0: v = (1 - a) v + a (|v| / |F|) F, and when npos > n_min: dt = min(dt f_inc, dt_max), a *= f_a;  npos += 1;
 *              else: v = 0, a = a_start, dt *= f_dec, npos = 0;  then v += dt F, dr = dt v, dr *= maxstep / |dr| when |dr| > maxstep (over all
 *              rows), frac = pymod1(frac + dr_x L^-1) with the L from before the move, L += dr_L / c_b, steps += 1.
 * MI_EINVAL: as mi_relax_init, and a handle whose largest crystal has more than MI_RELAX_MAX_ROWS - 3 atoms. */
int mi_relax_step(mi_batch* b, const mi_relax_params* params_host, int P, int p, float* frac, float* lattices, float* vel_x, float* vel_l,
                  float* fstate, int* istate, const float* g_frac, const float* g_lat, const float* out, void* stream);

/* mi_relax_run: `steps` iterations of { mi_scalar_input_grad at time t_all = 0 with g_types = NULL on (atom_types, frac, lattices) and the
 * seed d_out of mi_relax_init;  mi_relax_step }, enqueued on one stream from a state mi_relax_init (or an earlier run) left; finish != 0:
 * one more launch marks what is still ACTIVE as EXHAUSTED.  atom_types is read only; out [B][P], g_frac [N][3], g_lat [B][9] are the
 * caller's work arrays.  The refusals are mi_scalar_input_grad's, by name, before anything is enqueued, and mi_relax_step's; steps < 0.
 * B = 0 or steps = 0: MI_OK, nothing is launched. */
int mi_relax_run(mi_net* net, mi_batch* b, const mi_relax_params* params_host, const float* atom_types, float* frac, float* lattices,
                 const float* time_freqs, const float* W, const float* bias, int P, int p, const float* d_out, float* out, float* g_frac,
                 float* g_lat, float* vel_x, float* vel_l, float* fstate, int* istate, int steps, int finish, void* stream);

#ifdef __cplusplus
}
#endif

#endif
