/*
 * matinvent_hip_sym.h -- space-group operations, point group and primitive cell of the crystals of a prepared set: the
 * structure matcher of matinvent_hip_smatch.h run on (b, b) with a rigid metric, a nearest-atom test instead of an optimal assignment and
 * every accepted (map, translation) item kept.  Same conventions (device pointers, int32 indices, 0 or a negative MI_E* code, nothing read
 * back, everything enqueued on the caller's stream; no atomics, no scratch, no matrix pipe); a header of its own because the entry lists of
 * the other headers are fixed.  All arithmetic is float64 or exact integers; matinvent_amd/csrc/sym_ops.h holds every formula and reuses
 * sm_lattice.h and sm_assign.h.  Not built: the space-group number or Hall symbol, standardised cells, Wyckoff positions.
 *
 * Find (one 256-thread workgroup per crystal).  tol[b] is the position and length tolerance of crystal b in the prepared set's units
 * (unit volume per atom): the host passes symprec / (V_b / n_b)^(1/3).  Lattice maps of the reduced cell L onto itself: the matcher's box,
 * candidates and triples in the matcher's order, with the length rule | |k L| - |a_i| | <= tol, the matcher's angle rule and integer
 * determinant +-1.  Per (map W, translation j) item, in map-major order: f' = wrap(f W^-1), t = f[rarest species' atom j] - f'[rarest
 * species' first atom]; the item is an operation iff every atom's image f' + t has an atom of its species within tol (metric G = L L^T,
 * smallest distance over the 27 neighbouring images, the nearest atom the first minimum in ascending order) and the atom -> atom map is a
 * bijection.  All atoms within tol but no bijection: rejected, and the crystal's status gains MI_SYM_AMBIGUOUS.  Accepted operations are
 * written in that order up to MI_SYM_MAX_OPS as rot (W), trans (t wrapped to [0, 1)) and dev (the largest atom-to-image distance); past the
 * cap the counts stay exact and the status gains MI_SYM_OPS_CAP.  The operations with W = I are the pure translations (at most 64):
 * ptrans holds wrap(t - mean displacement) of each.  The distinct W of the operations are classified by (determinant, trace) into the
 * classes -6, -4, -3, -2, -1, 1, 2, 3, 4, 6 (rot_hist in that order); the histogram names the point group (pg_index 1 .. 32 in the order
 * 1, -1, 2, m, 2/m, 222, mm2, mmm, 4, -4, 4/m, 422, 4mm, -42m, 4/mmm, 3, -3, 32, 3m, -3m, 6, -6, 6/m, 622, 6mm, -6m2, 6/mmm, 23, m-3,
 * 432, -43m, m-3m; 0: none of them) and the crystal system (1 triclinic .. 7 cubic; 0 with pg_index 0).  n_ops != pg_order x n_trans, a W
 * of no class, or a histogram of no point group: MI_SYM_NOT_A_GROUP.
 *
 * info row [MI_SYM_INFO]: n_ops, n_trans, n_maps, pg_order, pg_index, crystal_system, has_inversion, status.  The status is a bit field
 * over MI_SYM_OK.  A crystal whose prepare status is not OK, or whose tol is not in [0, 1], or without a map list (box or map cap) gets its
 * status, a zeroed info row and a zeroed rot_hist row, and nothing else is written for it.
 *
 * Primitive (one wave per crystal, a scan launch, one wave per crystal).  Candidate basis vectors: the refined pure translations, every
 * component moved to [-1/2, 1/2), then the three unit vectors; the first triple i < j < k in nested ascending order with
 * | |det| n_trans - 1 | < 0.1 generates the translation lattice.  The primitive cell is that triple times the reduced cell in the
 * caller's scale (T x the caller's float32 cell, T the transform of mi_sm_prepare, recomputed here by the same function); the kept atoms
 * are the lowest-index member of each translation orbit, in the caller's order, their coordinates carried into the new basis and wrapped.
 * Outputs in the caller's layout, compacted: prim_offsets [B + 1], types, frac [.][3] float32, lat [B][9] float32 (mi_sm_prepare consumes
 * them, N the upper bound).  A crystal with n_trans = 1 or a find status other than OK or MI_SYM_OPS_CAP (past the cap the pure
 * translations are still all there) is copied unchanged, bit for bit; no triple, or orbits that are not n / n_trans: MI_SYM_PRIM_FAIL and
 * copied unchanged.  prim_status is the find status, with MI_SYM_PRIM_FAIL added.  A crystal whose offsets the prepare guard rejected
 * contributes no atoms.
 */
#ifndef MATINVENT_HIP_SYM_H
#define MATINVENT_HIP_SYM_H

#include "matinvent_hip_smatch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_SYM_MAX_OPS 192
#define MI_SYM_MAX_TRANS 64
#define MI_SYM_INFO 8
#define MI_SYM_CLASSES 10

#define MI_SYM_OK 0
#define MI_SYM_NOT_PREPARED 1
#define MI_SYM_BOX_CAP 2
#define MI_SYM_MAP_CAP 4
#define MI_SYM_NO_LATTICE 8
#define MI_SYM_AMBIGUOUS 16
#define MI_SYM_OPS_CAP 32
#define MI_SYM_NOT_A_GROUP 64
#define MI_SYM_PRIM_FAIL 128
#define MI_SYM_BAD_TOL 256

typedef struct mi_sym_out {
    int* info;      /* [B][8]: n_ops, n_trans, n_maps, pg_order, pg_index, crystal_system, has_inversion, status */
    int* rot_hist;  /* [B][10]: distinct rotation parts of class -6, -4, -3, -2, -1, 1, 2, 3, 4, 6 */
    int* rot;       /* [B][192][9]: W of the operations, in order */
    double* trans;  /* [B][192][3]: t wrapped to [0, 1) */
    double* dev;    /* [B][192]: the largest atom-to-image distance */
    double* ptrans; /* [B][64][3]: the refined pure translations, the identity first */
} mi_sym_out;

typedef struct mi_sym_prim_args {
    mi_sm_prepared set;     /* the prepared set mi_sym_find read */
    const int* types;       /* [N] the caller's arrays mi_sm_prepare read */
    const float* frac;      /* [N][3] */
    const float* lat;       /* [B][9] */
    const int* sym_info;    /* [B][8] of mi_sym_find */
    const double* ptrans;   /* [B][64][3] of mi_sym_find */
    int* ws_types;          /* [N] workspace */
    float* ws_frac;         /* [N][3] workspace */
    int* prim_count;        /* [B] kept atoms */
    int* prim_status;       /* [B] */
    double* prim_det;       /* [B] |det| of the chosen triple (1 for a crystal copied unchanged) */
    int* prim_offsets;      /* [B + 1] */
    int* out_types;         /* [N] */
    float* out_frac;        /* [N][3] */
    float* out_lat;         /* [B][9] */
} mi_sym_prim_args;

/* mi_sym_find: one launch on `stream`.  MI_EINVAL before anything is enqueued: a null pointer, a negative count, cos_tol outside (0, 1].
 * B == 0: MI_OK without a launch. */
int mi_sym_find(const mi_sm_prepared* set, const double* tol, double cos_tol, const mi_sym_out* out, void* stream);

/* mi_sym_primitive: three launches on `stream` (reduce into the workspace, scan the counts, gather), no host read between them.
 * MI_EINVAL: a null pointer, a negative count.  B == 0: MI_OK without a launch. */
int mi_sym_primitive(const mi_sym_prim_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif
