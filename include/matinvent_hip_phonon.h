/*
 * matinvent_hip_phonon.h -- PHONONS ON A Q-MESH of a learned energy from displacements of the HOME CELL of a supercell: force constants,
 * dynamical matrices at any q, their eigenvalues and the harmonic thermodynamics per primitive cell (phonons.py).  Same
 * conventions as matinvent_hip_vib.h, whose entries mi_vib_run_chunk (the gradients) and mi_sym_eigvals (the eigenvalues) are called as
 * they stand; a header of its own because the entry lists of the other headers are fixed.
 *
 * A primitive record of n atoms is replicated reps = (a, b, c) times, N = a b c, into a supercell of N_s = n N atoms in
 * structure.make_supercell's order: atom (I, j) has index I n + j, the images I = (I_a b + I_b) c + I_c in lexicographic order, image 0
 * (the home cell) first.  Only the home cell's atoms are displaced: plan entries c = 6 i + 2 d + s with i < n on the supercell as source,
 * so mi_vib_collect fills the 6 n rows Gc [6 n][3 N_s] and nothing else.  Behind them, float64 (csrc/phonon_fc.h holds every formula, host
 * and device; no transcendental function is evaluated on the device):
 *     Phi[(i, d)][(I, j, e)] = (Gc[6 i + 2 d][3 (I n + j) + e] - Gc[6 i + 2 d + 1][..]) / (2 h);
 *     the index symmetry Phi(0 i d; I j e) = Phi(0 j e; -I i d), -I modulo reps per axis: asym = max |Phi - Phi'| / max |Phi|, then
 *     Phi <- (Phi + Phi') / 2;  the acoustic sum rule: block (0 i; 0 i) = -sum over (I, j) != (0, i), ascending, symmetrised as a 3 x 3;
 *     the shortest-image table: for (i, I, j) a 27-bit mask over S in {-1, 0, 1}^3, bit s = 9 (S_a + 1) + 3 (S_b + 1) + (S_c + 1) set when
 *     |(x_(I,j) - x_(0,i) + S) L| <= d_min + tie_tol (x: the supercell's float32 coordinates widened, L its lattice, d_min the smallest of
 *     the 27): the matcher's 27-image search, so a supercell so skewed that the nearest image lies outside it is not served;
 *     D(q)[(i, d)][(j, e)] = (sum_I Phi(0 i d; I j e) (1 / mult) sum_{S in mask} e^{2 pi i q . (I + S o reps)}) / sqrt(m_i m_j), I and
 *     the bits ascending -- the lattice-vector phase convention, q in fractional reciprocal coordinates of the primitive cell.  The phase
 *     is the product (t_a t_b) t_c of three entries of a HOST table e^{2 pi i q_d r_d}, r_d = I_d + S_d reps_d = -reps_d .. 2 reps_d - 1;
 *     herm = max(|A - A^T|, |B + B^T|) / max(|A|, |B|) for D = A + i B;  D <- (D + D^H) / 2;  the real symmetric embedding
 *     [[A, -B], [B, A]] of order 6 n, whose eigenvalues (mi_sym_eigvals) are those of D, each twice;
 *     lambda_k = (ev[2 k] + ev[2 k + 1]) / 2, pair_gap = max (ev[2 k + 1] - ev[2 k]) / max |ev|;  frequencies, counts, c_v and the
 *     zero-point energy by vib_dynmat.h's functions, each q with its integer weight, divided by the weights' sum: per primitive cell.
 * No entry synchronises with the host, none uses atomics, scratch or the matrix pipe, and every sum is a serial loop whose order is a
 * function of the crystal's atom count and reps alone: a crystal has the same bits wherever it sits in whatever batch.
 *
 * The workspace of B supercells (doubles; mi_phonon_workspace gives the per-crystal base o_b):
 *     Gc [6 n][3 N_s] at o_b | Phi [3 n][3 N_s] at o_b + 18 n N_s | the masks, int32 [n][N][n], at o_b + 27 n N_s ((n N_s + 1) / 2 doubles).
 * The matrices of the (crystal, q) items and the eigen-solver's work copies are the caller's, at the offsets mi_sym_eigvals reads.
 */
#ifndef MATINVENT_HIP_PHONON_H
#define MATINVENT_HIP_PHONON_H

#include <stdint.h>

#include "matinvent_hip_vib.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_PHONON_MAX_PRIM 128    /* 6 n <= MI_EIG_MAX_M */
#define MI_PHONON_IMAGES 27

/* bytes of workspace for B supercells of num_atoms_host[b] atoms, each the reps_host [3]-fold replica of a primitive cell; offsets_host
 * [B + 1] (NULL: not wanted) gets o_b in doubles (o_B: the total).  MI_EINVAL: B < 0, a null list, a replica count < 1, an atom count
 * outside 1 .. MI_VIB_MAX_ATOMS, "reps does not divide the atom count", "6 n > MI_EIG_MAX_M". */
int64_t mi_phonon_workspace(const int* num_atoms_host, const int* reps_host, int B, int64_t* offsets_host);

typedef struct mi_phonon_fc_args {
    double* workspace;           /* Gc read, Phi and the masks written */
    const int64_t* ws_off;       /* [B] */
    const int* node_off;         /* [B + 1]: the supercells' atoms in `mass` and `frac` */
    const double* mass;          /* [N] amu; the home cell's are read */
    const float* frac;           /* [N][3] */
    const float* lat;            /* [B][9] */
    double* asym;                /* [B] */
    int* status;                 /* [B]: MI_VIB_OK or MI_VIB_BAD_INPUT (Phi and asym are NaN, the masks 0) */
    double h;
    double tie_tol;              /* Angstrom, finite and >= 0 */
    double det_min;              /* > 0 */
    int reps[3];
    int B;
    int max_atoms;               /* the largest atom count, 1 .. MI_VIB_MAX_ATOMS; a larger crystal is skipped (status MI_VIB_BAD_INPUT) */
} mi_phonon_fc_args;

/* mi_phonon_fc: one launch, one workgroup per crystal.  MI_VIB_BAD_INPUT: a non-finite gradient, lattice or home mass element,
 * |det L| < det_min, a home mass <= 0, an atom count that reps does not divide or whose primitive cell exceeds MI_PHONON_MAX_PRIM atoms
 * (nothing but status and asym is written for the last two).  MI_EINVAL: a null pointer, B < 0, h or det_min not finite and positive,
 * a bad tie_tol, a replica count < 1, max_atoms outside 1 .. MI_VIB_MAX_ATOMS.  B == 0: MI_OK without a launch. */
int mi_phonon_fc(const mi_phonon_fc_args* args, void* stream);

typedef struct mi_phonon_dynmat_args {
    const double* workspace;     /* Phi and the masks read */
    const int64_t* ws_off;       /* [B] */
    const int* node_off;         /* [B + 1] */
    const double* mass;          /* [N] */
    const int* fc_status;        /* [B], mi_phonon_fc's */
    const double* table;         /* [Q][6 (a + b + c)]: per q the axes in order, per axis 3 reps_d entries (re, im) of e^{2 pi i q_d r_d}, r_d ascending */
    const int* item_crystal;     /* [T] */
    const int* item_q;           /* [T] */
    double* mats;                /* item t: sizes[t]^2 doubles, row-major, at mats + mat_off[t] */
    const int64_t* mat_off;      /* [T] */
    const int* sizes;            /* [T]: 6 n of the item's crystal */
    double* herm;                /* [T] */
    int64_t table_len;           /* doubles in `table`: Q 6 (a + b + c) */
    int reps[3];
    int B, Q, T;
} mi_phonon_dynmat_args;

/* mi_phonon_dynmat: one launch, one workgroup per item.  An item whose crystal is not MI_VIB_OK, or whose size is not 6 n, gets a matrix
 * of NaN (mi_sym_eigvals answers MI_VIB_BAD_INPUT) and herm NaN; an item outside the crystals or the q list writes nothing.
 * MI_EINVAL: a null pointer, B, Q or T < 0, a replica count < 1, "the q-table has .. doubles".  T == 0: MI_OK without a launch. */
int mi_phonon_dynmat(const mi_phonon_dynmat_args* args, void* stream);

typedef struct mi_phonon_thermo_args {
    const double* evals;         /* item t: sizes[t] of them at evals + ev_off[t], ascending (mi_sym_eigvals') */
    const int64_t* ev_off;       /* [T], even */
    const int* sizes;            /* [T] */
    const int* eig_status;       /* [T] */
    const int* sweeps;           /* [T] */
    const double* herm_item;     /* [T], mi_phonon_dynmat's */
    const int* fc_status;        /* [B] */
    const int* item_off;         /* [B + 1]: the items of crystal b, contiguous and in the order of their q */
    const int* item_q;           /* [T] */
    const int* weight;           /* [Q]: >= 1 */
    double* lam;                 /* item t: sizes[t] / 2 at lam + ev_off[t] / 2, eV / (amu A^2) */
    double* freqs;               /* THz, the same layout; negative: imaginary */
    double* c_v;                 /* [B][K], in k_B per primitive cell */
    double* zpe;                 /* [B], eV per primitive cell */
    int* n_imag;                 /* [B]: weighted counts over the mesh */
    int* n_zero;                 /* [B] */
    double* min_freq;            /* [B] */
    int* min_q;                  /* [B]: the q of min_freq (the first that has it) */
    double* herm;                /* [B]: the largest of the items' */
    double* pair_gap;            /* [B] */
    int* sweeps_max;             /* [B] */
    int* status;                 /* [B]: fc_status when it is not MI_VIB_OK, else the largest eig_status; on anything but MI_VIB_OK the outputs are
                                    NaN and the counts -1 */
    double temps[MI_VIB_MAX_TEMPS];   /* K, finite and > 0 */
    double nu_cut;               /* THz, finite and >= 0 */
    int B, K, Q;                 /* K: 1 .. MI_VIB_MAX_TEMPS */
} mi_phonon_thermo_args;

/* mi_phonon_thermo: one launch, one wave per crystal.  Gamma's acoustic modes are not projected out: the sum rule makes them zero to
 * rounding and nu_cut counts them into n_zero.  MI_EINVAL: a null pointer, B or Q < 0, K outside 1 .. MI_VIB_MAX_TEMPS, a bad temperature or
 * nu_cut. */
int mi_phonon_thermo(const mi_phonon_thermo_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif
