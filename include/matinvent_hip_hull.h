/*
 * matinvent_hip_hull.h -- energy above the convex hull: for groups of query compositions, the energy per atom of the lower
 * convex hull of a device-resident bank of reference phases at each query's composition, its chemical potentials and the decomposition.
 * Same conventions as matinvent_hip_match.h (device pointers, CSR groups, int32 indices, 0 or a negative MI_E* code, nothing read back,
 * everything enqueued on the caller's stream); a header of its own because the entry lists of the other headers are fixed.  Every value is
 * float64.
 *
 * The problem.  A query has d distinct elements (1 <= d <= MI_HULL_MAX_ELEMS), atomic fractions c[d] (>= 0, sum 1) and an energy per atom
 * e_q.  Its candidates are bank rows whose element set is a subset of the query's: fractions x_i in the query's d coordinates, energy E_i.
 *     e_hull = min sum_i l_i E_i   subject to   sum_i l_i x_i = c,  l >= 0;        e_above = e_q - e_hull.
 * The query is not a candidate of itself, so e_above may be negative.
 *
 * Bank.  Row r: bank_nelem[r] elements, their atomic numbers bank_Z[r][0 .. n - 1] sorted ascending, their fractions bank_frac[r][..] and
 * bank_energy[r] per atom (NaN allowed: the row is never priced).
 *
 * Groups.  Group g is one element set: grp_nelem[g] = d, grp_Z[g][0 .. d - 1] strictly ascending; it owns the query positions
 * grp_q_off[g] .. grp_q_off[g + 1] - 1 of q_idx (rows of query_c / query_e and of every output) and the candidate positions
 * grp_c_off[g] .. grp_c_off[g + 1] - 1 of c_idx (rows of the bank).  A query's coordinates are its group's element order.
 *
 * The algorithm (matinvent_amd/csrc/hull_simplex.h holds every formula): a revised simplex from the elemental vertex.  The basis starts
 * with, per element, the pure candidate (x_ik == 1) of lowest finite energy, ties to the lowest list position; B^-1 = I, l = c.  Each
 * iteration: y = E_B B^-1; r_i = E_i - sum_k y_k x_ik (k ascending, each product and each addition rounded separately) over the
 * non-basic candidates of finite energy; the smallest enters, ties to the lowest list position, unless it is >= -MI_HULL_EPS
 * (MI_HULL_OK); u = B^-1 x_j; the smallest l_k / u_k over u_k > MI_HULL_EPS leaves, ties to the lowest k (none: MI_HULL_UNBOUNDED);
 * l, clamped at 0 from below, and B^-1 are updated in product form.  MI_HULL_ITER_CAP after MI_HULL_MAX_ITERS pivots.
 *
 * Work.  Two launches.  A staging kernel (one 256-thread workgroup per group) writes the group's candidates as a dense
 * structure-of-arrays block -- d columns of fractions in the group's element order, then the energies -- into the workspace.  A solve
 * kernel (one 256-thread workgroup per query position) prices the block with its threads striding over the candidates, reduces
 * (value, position) through a fixed tree, and lets one lane do the d x d part; the block sits in LDS when (d + 1) x candidates <=
 * MI_HULL_LDS_DOUBLES and is streamed from global memory otherwise.  Both paths give the same bits: r_i is a function of its row and y.
 * No atomics, no scratch, no matrix pipe.
 *
 * Guard.  A candidate whose index is outside 0 .. M - 1, whose row has n_elem outside 1 .. 8, an element outside the group's set or a
 * fraction that is not finite is skipped (never priced, nothing read through a bad index) and the group's queries get
 * MI_HULL_FLAG_SKIPPED in `flags`.  A group whose element list is not 1 .. 8 strictly ascending numbers or whose offsets do not lie inside
 * the lists, and a query index outside 0 .. Q - 1, are skipped in the same way: those output rows keep what they held.
 *
 * Outputs per query row.  e_hull = y . c; e_above; chempot[8] = y; decomp_idx[8] = the bank rows of the final basis (-1 past d);
 * decomp_frac[8] = l (0 past d); iters = pivots; status.  MI_HULL_NO_TERMINAL (an element without a pure candidate of finite energy) and
 * MI_HULL_BAD_QUERY (a fraction that is negative or not finite): e_hull, e_above, chempot are NaN, decomp_idx -1, decomp_frac 0.
 */
#ifndef MATINVENT_HIP_HULL_H
#define MATINVENT_HIP_HULL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_HULL_MAX_ELEMS 8
#define MI_HULL_MAX_ITERS 256
#define MI_HULL_EPS 1e-12
#define MI_HULL_LDS_DOUBLES 4096 /* 32 KiB: the largest (d + 1) x candidates block that is staged in LDS */

#define MI_HULL_OK 0
#define MI_HULL_NO_TERMINAL 1
#define MI_HULL_UNBOUNDED 2
#define MI_HULL_ITER_CAP 3
#define MI_HULL_BAD_QUERY 4

#define MI_HULL_FLAG_SKIPPED 1

typedef struct mi_hull_args {
    /* the bank */
    const int* bank_nelem;      /* [M] */
    const int* bank_Z;          /* [M][8] */
    const double* bank_frac;    /* [M][8] */
    const double* bank_energy;  /* [M] */
    /* the groups (CSR) */
    const int* grp_nelem;       /* [G] */
    const int* grp_Z;           /* [G][8] */
    const int* grp_q_off;       /* [G + 1] */
    const int* q_idx;           /* [nnz_q] */
    const int* grp_c_off;       /* [G + 1] */
    const int* c_idx;           /* [nnz_c] */
    /* the queries */
    const double* query_c;      /* [Q][8], in the group's element order */
    const double* query_e;      /* [Q]; NaN gives e_above NaN, everything else is computed */
    void* workspace;            /* mi_hull_workspace(G, nnz_q, nnz_c) bytes, 16-byte aligned */
    /* outputs, per query row */
    double* e_hull;             /* [Q] */
    double* e_above;            /* [Q] */
    double* chempot;            /* [Q][8] */
    double* decomp_frac;        /* [Q][8] */
    int* decomp_idx;            /* [Q][8] */
    int* iters;                 /* [Q] */
    int* status;                /* [Q] */
    int* flags;                 /* [Q] */
    int M, G, Q, nnz_q, nnz_c;
    int max_elems;              /* the largest grp_nelem, 1 .. MI_HULL_MAX_ELEMS */
    int no_lds;                 /* debug: non-zero streams every block from global memory */
} mi_hull_args;

/* bytes of staging memory for G groups, nnz_q query positions and nnz_c candidate positions; a negative count: MI_EINVAL */
int64_t mi_hull_workspace(int G, int nnz_q, int nnz_c);

/* mi_hull_above: one fill of the workspace's maps and two launches on `stream`, nothing read back.  MI_EINVAL before anything is
 * enqueued: a null pointer, a negative count, max_elems outside 1 .. MI_HULL_MAX_ELEMS, a workspace that is not 16-byte aligned.
 * G == 0, Q == 0 or nnz_q == 0: MI_OK without a launch. */
int mi_hull_above(const mi_hull_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif
