/*
 * matinvent_hip_sym_conv.h -- the conventional cell, the centring and the Bravais lattice of the primitive crystals of a prepared set
 * (DESIGN 53), from the operations mi_sym_find returned for that set.  Same conventions as matinvent_hip_sym.h (device pointers, int32
 * indices, 0 or a negative MI_E* code, nothing read back, everything enqueued on the caller's stream; no atomics, no scratch, no matrix
 * pipe); a header of its own because the entry lists of the other headers are fixed.  All arithmetic is float64 or exact integers;
 * matinvent_amd/csrc/sym_conv.h holds every formula.  Not built: the space-group number or Hall symbol, Wyckoff positions and site orbits,
 * idealised cell parameters, the re-setting of a monoclinic A or I cell to C.
 *
 * The crystals are expected primitive (mi_sym_primitive, prepared and analysed again): with pure translations left in a crystal the
 * basis below spans the cell given, not the lattice.
 *
 * Basis (one wave per crystal).  The distinct rotation parts W in operation order give proper parts P = det(W) W, their order n in
 * {1, 2, 3, 4, 6} by repeated multiplication, S = I + P + .. + P^(n-1) and the axis (the first non-zero row of S over its gcd, its first
 * non-zero entry positive); an integer row k is perpendicular to the axis iff k S = 0.  M [3][3] (rows: the conventional vectors in the
 * reduced primitive basis) by crystal_system of the find info row -- triclinic: I; monoclinic: b the one two-fold axis, a and c the
 * shortest and the shortest non-parallel k of [-2, 2]^3 with k S = 0, c's sign such that a.c <= 0; orthorhombic: the three two-fold axes,
 * a <= b <= c, a cell centred on one face permuted so that the face is ab; tetragonal: c the four-fold axis, a the shortest k
 * perpendicular to it, b = a P4 (P4 the first proper part of order 4); trigonal and hexagonal: c the three-fold axis, a the shortest
 * perpendicular k, b = a P3 (the first proper part of order 3, or the square of the first of order 6), a rhombohedral cell turned
 * obverse; cubic: the three four-fold axes, without them the three two-fold ones, in descending lexicographic order.  "Shortest" is the
 * minimum of (k G k^T, index in the box), G = L L^T of the prepared cell, the lower index the lexicographically larger k.  det M < 0:
 * c is negated (b in the monoclinic system, where c's sign is taken).  mult = det M; the centring vectors are the distinct k adj(M) mod
 * mult, numerators over mult, ascending with zero first; their set names the centring (1 P, 2 A, 3 B, 4 C, 5 I, 6 F, 7 R) and, with the
 * system, the Bravais lattice (1 .. 14 in the order aP mP mS oP oS oI oF tP tI hR hP cP cI cF).
 *
 * conv_info row [8]: bravais, centring, mult, crystal_system, n_axes, max |M|, 0, status.  The status is the find status, with
 * MI_SYM_CONV_FAIL added when the find status is not MI_SYM_OK, an axis count does not fit the system, mult is not one of the system's, the
 * vector set is no known centring, a needed vector is not in the box, or the prepare transform is too large for exact 32-bit adjugates.
 * Such a crystal has bravais 0, centring 0, mult 1, M = I and is copied unchanged, bit for bit.  A crystal the prepare guard rejected has
 * conv_count 0: no atom and no cell is written for it.
 *
 * Outputs in the caller's layout: conv_offsets [B + 1], types and frac [.][3] float32 atom-major (the mult copies of an atom are
 * consecutive, in centring-vector order: wrap((f adj(M T) + v_j) / mult), f the caller's float32 coordinates, T the transform of
 * mi_sm_prepare recomputed by the same function), lat [B][9] float32 = M x T x the caller's cell, formed in float64 and rounded once.  The
 * atom arrays hold 4 N rows.
 */
#ifndef MATINVENT_HIP_SYM_CONV_H
#define MATINVENT_HIP_SYM_CONV_H

#include "matinvent_hip_sym.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_SYM_CONV_FAIL 512
#define MI_SYM_CONV_INFO 8
#define MI_SYM_CONV_MAX_MULT 4

typedef struct mi_sym_conv_args {
    mi_sm_prepared set;     /* the prepared set of the primitive crystals, which mi_sym_find read */
    const int* types;       /* [N] the caller's arrays mi_sm_prepare read */
    const float* frac;      /* [N][3] */
    const float* lat;       /* [B][9] */
    const int* sym_info;    /* [B][8] of mi_sym_find */
    const int* sym_rot;     /* [B][192][9] of mi_sym_find */
    int* ws_adj;            /* [B][9] workspace: adj(M T) */
    int* conv_info;         /* [B][8]: bravais, centring, mult, crystal_system, n_axes, max |M|, 0, status */
    int* conv_M;            /* [B][9] */
    int* conv_cvec;         /* [B][4][3] numerators over mult */
    int* conv_count;        /* [B] mult x n */
    int* conv_offsets;      /* [B + 1] */
    int* out_types;         /* [4 N] */
    float* out_frac;        /* [4 N][3] */
    float* out_lat;         /* [B][9] */
} mi_sym_conv_args;

/* mi_sym_conventional: three launches on `stream` (basis, scan of the counts, gather), no host read between them.  MI_EINVAL before
 * anything is enqueued: a null pointer, a negative count, 4 N beyond int32.  B == 0: MI_OK without a launch. */
int mi_sym_conventional(const mi_sym_conv_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif
