/*
 * matinvent_hip_vib.h -- GAMMA-POINT VIBRATIONS of a learned energy: normal modes, dynamical stability and the harmonic heat capacity
 * (vibrations.py).  Same conventions as matinvent_hip.h (device pointers unless a name ends in `_host`, int32 indices unless
 * said otherwise, 0 or a negative MI_E* code); a header of its own because the entry lists of the other headers are fixed.
 *
 * The energy is column p of the property predictor (matinvent_hip_scalar.h), its gradient mi_scalar_input_grad's, the convention
 * matinvent_hip_relax.h's: lattice rows are cell vectors, cart = frac L, dE / dr_j = s_b g_frac[j] L^-T with s_b = scale (x n when
 * per_atom).  The Hessian is the central difference of that gradient over 6 n displaced copies of a crystal of n atoms,
 *     copy c = 6 i + 2 d + s:   frac[i] = pymod1(frac[i] + (s ? -h : +h) e_d L^-1),   everything else copied,
 *     H[(i, d)][(j, e)] = (Gc[c+][j][e] - Gc[c-][j][e]) / (2 h),
 * and everything behind it is float64 (csrc/vib_dynmat.h and csrc/sym_jacobi.h hold every formula, host and device):
 *     asym = max |H - H^T| / max |H|;  H <- (H + H^T) / 2;  the acoustic sum rule: the diagonal 3 x 3 block of atom i = -sum_{j != i} of its
 *     row blocks, symmetrised;  D = H / sqrt(m_i m_j);  three Householder reflectors Q take the normalised translations to the first three
 *     unit vectors;  the vibrational matrix R is the trailing (3 n - 3)^2 block of Q D Q^T, symmetrised (n = 1: no modes);
 *     eigenvalues by cyclic Jacobi in the round-robin ordering, ascending;  nu_k = sign(l_k) sqrt|l_k| 15.633304 THz (eV, A, amu);
 *     c_v(T) / k_B = sum x^2 e^-x / (1 - e^-x)^2, x = h nu / (k_B T), and zpe = 1/2 sum h nu over the real modes above nu_cut.
 * No entry synchronises with the host, none uses atomics, scratch or the matrix pipe, and every sum is a serial loop whose order is a
 * function of the crystal's atom count alone: a crystal has the same bits wherever it sits in whatever batch.
 *
 * The workspace of B source crystals (doubles; mi_vib_workspace gives the per-crystal base o_b):
 *     Gc [6 n][3 n] at o_b | W [3 n][3 n] at o_b + 18 n^2 | R [M][M] at o_b + 27 n^2 | the eigen-solver's copy at o_b + 27 n^2 + M^2,   M = 3 n - 3.
 */
#ifndef MATINVENT_HIP_VIB_H
#define MATINVENT_HIP_VIB_H

#include <stdint.h>

#include "matinvent_hip_relax.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_VIB_OK 0
#define MI_VIB_NO_CONVERGENCE 1   /* rotations were still made in sweep MI_EIG_MAX_SWEEPS */
#define MI_VIB_BAD_INPUT 2        /* a non-finite gradient, lattice or mass element, |det L| < det_min, a mass <= 0, a non-finite matrix element */

/* 256, not the 512 the workspace would allow (57 MB per crystal there): one workgroup diagonalises one matrix, the work grows with the cube
 * of its order, and above 256 atoms (order 765) one matrix would hold a compute unit for minutes */
#define MI_VIB_MAX_ATOMS 256
#define MI_VIB_MAX_TEMPS 8
#define MI_EIG_MAX_SWEEPS 30
#define MI_EIG_LDS_MAX_M 128      /* 8 M^2 <= 128 KiB: the matrix is rotated in LDS (n <= 43); above, in the work copy in global memory */
#define MI_EIG_MAX_M 768

/* bytes of workspace for B crystals of num_atoms_host[b] atoms; offsets_host [B + 1] (NULL: not wanted) gets o_b in doubles (o_B: the total).
 * MI_EINVAL: B < 0, a null list, an atom count outside 1 .. MI_VIB_MAX_ATOMS. */
int64_t mi_vib_workspace(const int* num_atoms_host, int B, int64_t* offsets_host);

typedef struct mi_vib_chunk_args {
    /* the source state: Bs crystals, read only */
    const float* src_types;      /* [Ns][100] */
    const float* src_frac;       /* [Ns][3] */
    const float* src_lat;        /* [Bs][9] */
    const int* src_node_off;     /* [Bs + 1] */
    int Bs;
    /* the chunk plan, one entry per crystal of the chunk's handle: displaced copy plan_copy[k] of source crystal plan_src[k] */
    const int* plan_src;         /* [Bc] */
    const int* plan_copy;        /* [Bc] */
    /* the chunk's state, written by mi_vib_displace (16-byte aligned) */
    float* types;                /* [Nc][100] */
    float* frac;                 /* [Nc][3] */
    float* lat;                  /* [Bc][9] */
    /* the chunk's gradient, read by mi_vib_collect */
    float* g_frac;               /* [Nc][3] */
    double* workspace;           /* mi_vib_workspace of the SOURCE crystals */
    const int64_t* ws_off;       /* [Bs]: o_b */
    double h;                    /* the displacement in Angstrom, finite and > 0 */
    double scale;                /* std[p] of the property's normaliser, finite and > 0 */
    double det_min;              /* > 0 */
    int per_atom;                /* 1: column p is an energy per atom */
} mi_vib_chunk_args;

/* mi_vib_displace: the chunk's frac, lat and type rows from the source state and the plan -- one launch, one workgroup per copy, the type
 * rows moved with 16-byte accesses.  `b` is a classic handle made for the copies' atom counts.  A plan entry outside the source, a copy
 * index outside 0 .. 6 n - 1 or an atom count that is not the source crystal's writes nothing (nothing is read through a bad index); a
 * source lattice that is not finite or has |det L| < det_min is copied with its coordinates as they are.
 * MI_EINVAL: a null handle or argument, a pooled handle, h / scale / det_min not finite and positive, Bs < 0, misaligned chunk arrays. */
int mi_vib_displace(mi_batch* b, const mi_vib_chunk_args* args, void* stream);

/* mi_vib_collect: row plan_copy[k] of Gc of source crystal plan_src[k] from the chunk's g_frac and lat: Gc[c][3 j + e] =
 * s_b (g_frac[j] . row e of L^-1), widened first.  A bad lattice gives a row of NaN, a non-finite gradient element passes through:
 * mi_vib_dynmat answers both with MI_VIB_BAD_INPUT.  One launch.  The refusals are mi_vib_displace's. */
int mi_vib_collect(mi_batch* b, const mi_vib_chunk_args* args, void* stream);

/* mi_vib_run_chunk: mi_vib_displace;  mi_scalar_input_grad at time t_all = 0 with g_types = NULL on the chunk's state and the caller's
 * seed d_out [Bc][P] (+1 in column p, 0 elsewhere) -> out [Bc][P], args->g_frac, g_lat [Bc][9];  mi_vib_collect -- enqueued on one
 * stream.  The refusals are mi_scalar_input_grad's, by name, before anything is enqueued, and mi_vib_displace's. */
int mi_vib_run_chunk(mi_net* net, mi_batch* b, const mi_vib_chunk_args* args, const float* time_freqs, const float* W, const float* bias, int P,
                     const float* d_out, float* out, float* g_lat, void* stream);

typedef struct mi_vib_dynmat_args {
    double* workspace;           /* Gc read, W used, R written */
    const int64_t* ws_off;       /* [B] */
    const int* node_off;         /* [B + 1]: the crystals' atoms in `mass` */
    const double* mass;          /* [N] amu */
    double* asym;                /* [B] */
    int* status;                 /* [B]: MI_VIB_OK or MI_VIB_BAD_INPUT (R and asym are NaN) */
    double h;
    int B;
    int max_atoms;               /* the largest atom count, 1 .. MI_VIB_MAX_ATOMS; a larger crystal is skipped (status MI_VIB_BAD_INPUT) */
} mi_vib_dynmat_args;

/* mi_vib_dynmat: one launch, one workgroup per crystal.  MI_EINVAL: a null pointer, B < 0, h not finite and positive, max_atoms outside
 * 1 .. MI_VIB_MAX_ATOMS.  B == 0: MI_OK without a launch. */
int mi_vib_dynmat(const mi_vib_dynmat_args* args, void* stream);

typedef struct mi_sym_eig_args {
    const double* mats;          /* matrix b: sizes[b]^2 doubles, row-major, at mats + mat_off[b]; read only */
    const int64_t* mat_off;      /* [B] */
    const int* sizes;            /* [B]: 0 .. max_size; a size outside it: status MI_VIB_BAD_INPUT, nothing else written */
    double* work;                /* the copy that is rotated when a matrix does not sit in LDS, at work + work_off[b]; NULL allowed when
                                    max_size <= MI_EIG_LDS_MAX_M and no_lds == 0 */
    const int64_t* work_off;     /* [B]; NULL: mat_off */
    double* evals;               /* sizes[b] doubles at evals + ev_off[b], ascending */
    const int64_t* ev_off;       /* [B] */
    int* sweeps;                 /* [B]: the sweeps that rotated */
    int* status;                 /* [B]: MI_VIB_OK, MI_VIB_NO_CONVERGENCE (the diagonal reached is written) or MI_VIB_BAD_INPUT (NaN) */
    int B;
    int max_size;                /* 0 .. MI_EIG_MAX_M */
    int no_lds;                  /* debug: non-zero rotates every matrix in global memory */
} mi_sym_eig_args;

/* mi_sym_eigvals: the eigenvalues of B real symmetric matrices of ragged sizes -- one launch, one workgroup per matrix; only the upper
 * triangle decides a rotation.  Usable on its own.  MI_EINVAL: a null pointer, B < 0, max_size outside 0 .. MI_EIG_MAX_M, no work array
 * where one is needed.  B == 0 or max_size == 0: sweeps 0 and status MI_VIB_OK are still written (one launch) unless B == 0. */
int mi_sym_eigvals(const mi_sym_eig_args* args, void* stream);

typedef struct mi_vib_thermo_args {
    const double* evals;         /* at evals + ev_off[b], sizes[b] of them, ascending */
    const int64_t* ev_off;       /* [B] */
    const int* sizes;            /* [B] */
    const int* eig_status;       /* [B] */
    const int* dyn_status;       /* [B], mi_vib_dynmat's; NULL: eigenvalues that did not come from it */
    double* freqs;               /* THz at freqs + ev_off[b]; negative: imaginary */
    double* c_v;                 /* [B][K], in k_B */
    double* zpe;                 /* [B], eV */
    int* n_imag;                 /* [B] */
    int* n_zero;                 /* [B] */
    int* status;                 /* [B]: dyn_status when it is not MI_VIB_OK (a crystal of one atom has no matrix element to carry its bad input
                                    to the solver), else eig_status; on anything but MI_VIB_OK the outputs are NaN and the counts -1 */
    double temps[MI_VIB_MAX_TEMPS];   /* K, finite and > 0 */
    double nu_cut;               /* THz, finite and >= 0 */
    int B, K;                    /* K: 1 .. MI_VIB_MAX_TEMPS */
} mi_vib_thermo_args;

/* mi_vib_thermo: one launch, one wave per crystal.  A mode with nu < -nu_cut counts in n_imag, one with |nu| <= nu_cut in n_zero; neither
 * contributes.  MI_EINVAL: a null pointer, B < 0, K outside 1 .. MI_VIB_MAX_TEMPS, a bad temperature or nu_cut. */
int mi_vib_thermo(const mi_vib_thermo_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif
