/*
 * matinvent_hip_elastic.h -- ELASTIC TENSOR AND MODULI of a learned energy: the stress of strained copies of a cell, the 6 x 6 tensor, its
 * inverse, the Voigt / Reuss / Hill averages and the Born stability count (elasticity.py).  Same conventions as matinvent_hip.h
 * (device pointers unless a name ends in `_host`, int32 indices unless said otherwise, 0 or a negative MI_E* code); a header of its own
 * because the entry lists of the other headers are fixed.
 *
 * The energy is column p of the property predictor (matinvent_hip_scalar.h), its gradient mi_scalar_input_grad's, the convention
 * matinvent_hip_relax.h's: lattice rows are cell vectors, cart = frac L, G = s_b g_lat[b] as a 3 x 3 matrix with s_b = scale (x n when
 * per_atom).  A symmetric strain eps takes the cell to L' = L (I + eps) at fixed fractional coordinates, formed in float64 and rounded once
 * to float32.  The stress of a cell is
 *     T = L'^T G',   sigma = (T + T^T) / (2 V'),   V' = |det L'|   (eV / A^3),      Voigt order 11, 22, 33, 23, 13, 12;
 * the network sees the lattice through L L^T only (g_lat = (M + M^T) L), so T is symmetric up to rounding: asym = max |T - T^T| / max |T| of
 * the unstrained copy is handed out.  A crystal has MI_ELASTIC_COPIES = 13 copies, whatever its size:
 *     copy c = 2 j + s (j = 0 .. 5, s = 0 / 1): eps = +-h E_j,  E_j = e_j e_j^T (j < 3),  (e_a e_b^T + e_b e_a^T) / 2 for the shear pairs (the
 *     engineering Voigt strain is exactly h);  copy 12: unstrained;
 *     C_ij = (sigma_i(+j) - sigma_i(-j)) / (2 h) x 160.2176634 GPa (exact from the SI value of e; h is the nominal one);
 *     asym_C = max |C - C^T| / max |C|;  C <- (C + C^T) / 2;  stress0 = sigma of copy 12 in GPa;  pressure = -tr sigma_0 / 3.
 * C IS THE DERIVATIVE OF THE CAUCHY STRESS AT THE GIVEN STRUCTURE.  Under a residual stress it is not the second derivative of the energy
 * (the two differ by terms linear in sigma_0): that is why stress0 and pressure are outputs.  With ion_steps = 0 the ions are clamped at
 * their fractional coordinates; with ion_steps > 0 every copy's ions are relaxed by FIRE at the fixed strained cell first.
 * From C and S = C^-1 (Gauss-Jordan with partial pivoting, ties to the lowest row), all float64 (csrc/elastic_fit.h holds every formula,
 * host and device):
 *     K_V = (C11 + C22 + C33 + 2 (C12 + C13 + C23)) / 9,            G_V = (C11 + C22 + C33 - (C12 + C13 + C23) + 3 (C44 + C55 + C66)) / 15,
 *     K_R = 1 / (S11 + S22 + S33 + 2 (S12 + S13 + S23)),            G_R = 15 / (4 (S11 + S22 + S33) - 4 (S12 + S13 + S23) + 3 (S44 + S55 + S66)),
 *     Hill = the mean of the two;  for each average E = 9 K G / (3 K + G),  nu = (3 K - 2 G) / (2 (3 K + G)),  the Pugh ratio K / G;
 *     the six eigenvalues of C by csrc/sym_jacobi.h's iteration (the bits of mi_sym_eigvals on the same matrix), ascending;
 *     n_negative = the negative ones (Born stability),  cond = max |lambda| / min |lambda| (no threshold is applied: the host decides).
 * No entry synchronises with the host, none uses atomics, scratch or the matrix pipe, and every sum is a serial loop in a fixed order: a
 * crystal has the same bits wherever it sits in whatever batch.
 *
 * The workspace of Bs source crystals: Bs x 13 rows of MI_ELASTIC_ROW = 8 doubles, row 13 b + c = sigma [6], V', flag of copy c of crystal b.
 */
#ifndef MATINVENT_HIP_ELASTIC_H
#define MATINVENT_HIP_ELASTIC_H

#include <stdint.h>

#include "matinvent_hip_vib.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_ELASTIC_OK 0
#define MI_ELASTIC_BAD_INPUT 1   /* a non-finite gradient or lattice element in any copy, |det L| < det_min, a copy whose ion relaxation FAILED: every output NaN, every count -1 */
#define MI_ELASTIC_SINGULAR 2    /* a zero or non-finite pivot: C, the Voigt values and the eigenvalues are kept, S and the Reuss and Hill values are NaN */

#define MI_ELASTIC_COPIES 13
#define MI_ELASTIC_ROW 8

typedef struct mi_elastic_chunk_args {
    /* the source state: Bs crystals, read only */
    const float* src_types;      /* [Ns][100] */
    const float* src_frac;       /* [Ns][3] */
    const float* src_lat;        /* [Bs][9] */
    const int* src_node_off;     /* [Bs + 1] */
    int Bs;
    /* the chunk plan, one entry per crystal of the chunk's handle: strained copy plan_copy[k] of source crystal plan_src[k] */
    const int* plan_src;         /* [Bc] */
    const int* plan_copy;        /* [Bc] */
    /* the chunk's state, written by mi_elastic_strain (16-byte aligned) */
    float* types;                /* [Nc][100] */
    float* frac;                 /* [Nc][3] */
    float* lat;                  /* [Bc][9] */
    /* the chunk's gradient, read by mi_elastic_collect (g_frac is the gradient's other half: work of mi_elastic_run_chunk only) */
    float* g_frac;               /* [Nc][3] */
    float* g_lat;                /* [Bc][9] */
    const int* istate;           /* [Bc][MI_RELAX_NI]: the chunk's mi_relax state; NULL: the ions are clamped */
    double* workspace;           /* [Bs][13][8] */
    double* asym;                /* [Bs]: written by the entry of copy 12 */
    double h;                    /* the strain, finite and > 0 */
    double scale;                /* std[p] of the property's normaliser, finite and > 0 */
    double det_min;              /* > 0 */
    int per_atom;                /* 1: column p is an energy per atom */
} mi_elastic_chunk_args;

/* mi_elastic_strain: the chunk's types, frac and lat from the source state and the plan -- one launch, one workgroup per copy, the type rows
 * moved with 16-byte accesses, frac copied bit for bit, lat = L (I + eps).  `b` is a classic handle made for the copies' atom counts.  A plan
 * entry outside the source, a copy index outside 0 .. 12 or an atom count that is not the source crystal's writes nothing (nothing is read
 * through a bad index); a source lattice that is not finite or has |det L| < det_min is copied as it is.
 * MI_EINVAL: a null handle or argument, a pooled handle, h / scale / det_min not finite and positive, Bs < 0, misaligned chunk arrays. */
int mi_elastic_strain(mi_batch* b, const mi_elastic_chunk_args* args, void* stream);

/* mi_elastic_collect: row plan_copy[k] of source crystal plan_src[k] from the chunk's g_lat and lat, widened first; the entry of copy 12
 * writes asym as well.  A bad lattice gives a row of NaN, a non-finite gradient element passes through; with istate, a copy whose status is
 * MI_RELAX_FAILED gives a row of NaN and one that is MI_RELAX_EXHAUSTED sets the row's flag to 1: mi_elastic_fit answers the first two
 * with MI_ELASTIC_BAD_INPUT and counts the third.  One launch.  The refusals are mi_elastic_strain's. */
int mi_elastic_collect(mi_batch* b, const mi_elastic_chunk_args* args, void* stream);

/* mi_elastic_run_chunk: mi_elastic_strain;  when ion_steps > 0, mi_relax_init and mi_relax_run(relax_cell = 0, steps = ion_steps, finish = 1)
 * on the chunk's state with the caller's vel_x [Nc][3], fstate [Bc][MI_RELAX_NF] and args->istate (which must not be NULL then; it is passed
 * to the collect step only when ion_steps > 0);  mi_scalar_input_grad at time t_all = 0 with g_types = NULL on the chunk's state and the
 * seed d_out [Bc][P] (+1 in column p, 0 elsewhere; mi_relax_init rewrites it) -> out [Bc][P], args->g_frac, args->g_lat;
 * mi_elastic_collect -- enqueued on one stream with no host wait.  Of relax_params_host (not read when ion_steps = 0) the FIRE constants,
 * fmax, cell_factor and n_min count; relax_cell is taken as 0 and scale, det_min and per_atom are args'.  The refusals are
 * mi_scalar_input_grad's and mi_relax_step's, by name, before anything is enqueued, and mi_elastic_strain's; ion_steps < 0. */
int mi_elastic_run_chunk(mi_net* net, mi_batch* b, const mi_elastic_chunk_args* args, const mi_relax_params* relax_params_host, int ion_steps,
                         const float* time_freqs, const float* W, const float* bias, int P, int p, float* d_out, float* out, float* vel_x,
                         float* fstate, void* stream);

typedef struct mi_elastic_fit_args {
    const double* workspace;     /* [B][13][8] */
    double* C;                   /* [B][36] GPa, symmetrised */
    double* S;                   /* [B][36] 1 / GPa */
    double* stress0;             /* [B][6] GPa */
    double* pressure;            /* [B] GPa */
    double* asym;                /* [B]: mi_elastic_collect's, kept; NaN on MI_ELASTIC_BAD_INPUT */
    double* asym_C;              /* [B] */
    double* moduli;              /* [B][3][5]: Voigt, Reuss, Hill x K, G, E (GPa), nu, K / G */
    double* evals;               /* [B][6] GPa, ascending */
    double* cond;                /* [B] */
    int* n_negative;             /* [B] */
    int* n_unrelaxed;            /* [B]: the copies whose ion relaxation was EXHAUSTED */
    int* status;                 /* [B] */
    double h;
    int B;
} mi_elastic_fit_args;

/* mi_elastic_fit: one launch, one wave per crystal.  MI_EINVAL: a null pointer, B < 0, h not finite and positive.  B == 0: MI_OK without
 * a launch. */
int mi_elastic_fit(const mi_elastic_fit_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif
