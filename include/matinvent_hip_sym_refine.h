/*
 * matinvent_hip_sym_refine.h -- the refined structure and the site orbits of the crystals of a prepared set, from the
 * operations mi_sym_find returned for that set: coordinates and cell projected onto the group that was found.  Same conventions as
 * matinvent_hip_sym.h (device pointers, int32 indices, 0 or a negative MI_E* code, nothing read back, everything enqueued on the caller's
 * stream; no atomics, no scratch, no matrix pipe); a header of its own because the entry lists of the other headers are fixed.  All
 * arithmetic is float64 or exact integers; matinvent_amd/csrc/sym_refine.h holds every formula.  Not built: Wyckoff letters, the
 * space-group number or Hall symbol, symmetry reduction of displaced sets, more than 64 atoms.
 *
 * Definition (one 256-thread workgroup per crystal), in the reduced basis of the prepared set, where operation k = 0 .. n_ops - 1 of
 * mi_sym_find is g_k(f) = f W_k^-1 + t_k (W_k^-1 the integer adjugate times the determinant) and the atoms are in prepared order:
 *   1. sigma_k(i) is the atom of i's species block nearest to wrap(x_i W_k^-1) + t_k (the finder's nearest-atom rule: metric of the
 *      prepared cell, 27 images, first minimum), r_k(i) the residual vector image - atom.  Every sigma_k must be a bijection.
 *   2. tbar_k = t_k - (sum_i r_k(i)) / n, the sum in ascending i: the least-squares translation of the map sigma_k.
 *   3. xbar_i = x_i + (sum_k d_k(i)) / n_ops, d_k(i) the 27-image minimum image of (x_sigma_k(i) - tbar_k) W_k - x_i, the sum in ascending k.
 *   4. With the caller's indices inside the crystal (through perm): orbit[i] is the lowest index among sigma_k(i), mult[i] the number of
 *      distinct sigma_k(i), site_order[i] = #{k : sigma_k(i) = i}; mult[i] x site_order[i] must be n_ops.
 *   5. L = T x the caller's float32 cell in float64 (T the transform of mi_sm_prepare, recomputed by the same function), G = L L^T,
 *      Gbar = (sum_k W_k G W_k^T) / n_ops in ascending k, Gc = T^-1 Gbar T^-T; the cell is the lower Cholesky factor of Gc (rows are the
 *      cell vectors, a along x, b in the xy plane), rounded to float32 once.  Every pivot must be positive.
 *   6. out_frac = wrap(xbar T) as float32 in [0, 1) (a float that rounds to 1 is 0), in the caller's atom order.
 *
 * refine_info row [8]: n_orbits, n_ops, 0, 0, 0, 0, 0, status.  The status is the find status, with MI_SYM_REFINE_FAIL added when the find
 * status is not MI_SYM_OK (MI_SYM_OPS_CAP included: past the cap the list is no group), a sigma_k is no bijection, an orbit check fails
 * or a pivot is not positive.  Such a crystal is copied unchanged, bit for bit, coordinates and cell, with orbit[i] = i, mult = 1,
 * site_order = 1, n_orbits = n and a zero refine_stat row.  A crystal with n_ops = 1 is copied the same way with the find status (OK).  A
 * crystal the prepare guard rejected gets its info row (0, 0, .., status with MI_SYM_NOT_PREPARED) and a zero refine_stat row; nothing is
 * written for its atoms or its cell.  refine_stat row [4], in the prepared set's units (unit volume per atom): the largest |xbar_i - x_i|,
 * the root mean square of the same, max |Gbar - G| / max |G|, the largest |r_k(i)|.  trans_ref rows k < n_ops hold tbar_k of a refined
 * crystal; no other row is written.
 */
#ifndef MATINVENT_HIP_SYM_REFINE_H
#define MATINVENT_HIP_SYM_REFINE_H

#include "matinvent_hip_sym.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_SYM_REFINE_FAIL 1024
#define MI_SYM_REFINE_INFO 8
#define MI_SYM_REFINE_STAT 4

typedef struct mi_sym_refine_args {
    mi_sm_prepared set;      /* the prepared set mi_sym_find read */
    const int* types;        /* [N] the caller's arrays mi_sm_prepare read */
    const float* frac;       /* [N][3] */
    const float* lat;        /* [B][9] */
    const int* sym_info;     /* [B][8] of mi_sym_find */
    const int* sym_rot;      /* [B][192][9] of mi_sym_find */
    const double* sym_trans; /* [B][192][3] of mi_sym_find */
    float* out_frac;         /* [N][3] */
    float* out_lat;          /* [B][9] */
    int* orbit;              /* [N] the lowest equivalent atom, an index inside the crystal */
    int* mult;               /* [N] atoms of the orbit */
    int* site_order;         /* [N] order of the site-symmetry group */
    double* trans_ref;       /* [B][192][3] */
    int* refine_info;        /* [B][8]: n_orbits, n_ops, 0, 0, 0, 0, 0, status */
    double* refine_stat;     /* [B][4]: max move, rms move, cell change, max residual */
} mi_sym_refine_args;

/* mi_sym_refine: one launch on `stream`.  MI_EINVAL before anything is enqueued: a null pointer, a negative count.  B == 0: MI_OK without
 * a launch. */
int mi_sym_refine(const mi_sym_refine_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif
