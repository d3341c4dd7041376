/*
 * matinvent_hip_smatch.h -- the structure matcher: for pairs of crystals of one composition, the lattice maps of the
 * candidate onto the query within (ltol, angle_tol), and over every (map, translation) the species-constrained optimal assignment of the
 * atoms; the result is the smallest RMS displacement, normalised by (V / n)^(1/3), with its map, translation and atom correspondence.
 * Same conventions as matinvent_hip_hull.h (device pointers, int32 indices, 0 or a negative MI_E* code, nothing read back, everything
 * enqueued on the caller's stream); a header of its own because the entry lists of the other headers are fixed.  All arithmetic is
 * float64 or exact integers; matinvent_amd/csrc/sm_lattice.h and sm_assign.h hold every formula.  It follows the algorithm of pymatgen's
 * StructureMatcher step by step and is not bit-compatible with it (DESIGN 49 lists the deviations); supercells, primitive-cell reduction
 * and the second acceptance criterion on max_dist are not built.
 *
 * Prepare (one wave per crystal).  Crystal b owns atoms offsets[b] .. offsets[b + 1] - 1 of types (atomic numbers 1 .. 118) and frac
 * (float32 fractional coordinates) and lat[b] (float32, rows are cell vectors).  The cell is reduced (a greedy Minkowski pair reduction
 * on an integer transform, tolerance-free), the coordinates are carried into the reduced basis and wrapped to [0, 1), the cell is scaled
 * to unit volume per atom, the atoms are sorted by ascending atomic number (stably) and the species block table and the rarest species
 * (fewest atoms, ties to the lowest atomic number) are recorded.  Status: MI_SM_PREP_*.  A crystal whose status is not OK has its info row
 * written and nothing else; nothing is read through offsets that do not satisfy 0 <= offsets[b] <= offsets[b + 1] <= N.
 *
 * Match (one 256-thread workgroup per pair).  Pair p compares query pair_q[p] of set a (the target) with candidate pair_c[p] of set b
 * (mapped onto it).  The sorted species lists must be equal.  Lattice maps: integer rows k with |k_i| <= floor((1 + ltol) max|axis_1|
 * |b2_i*|), in lexicographic order; k L2 is a candidate for axis i when | |k L2| / |axis_i| - 1 | <= ltol; triples of candidates in
 * nested ascending order whose three angles are within angle_tol of the target's (c c_t + sqrt(1 - c^2) sqrt(1 - c_t^2) >= cos_tol) and
 * whose integer determinant is +-1.  Per (map M, translation j) item, in map-major order: f2' = wrap(f2 M^-1), G = (L1 L1^T + (M L2)
 * (M L2)^T) / 2, t = f1[rarest species' atom j] - f2'[rarest species' first atom], the cost of an atom pair is the smallest
 * (D + k)^T G (D + k) over the 27 neighbouring images, each species block is assigned by shortest augmenting paths, and rms / max_dist are
 * taken about the mean displacement.  The pair's result is the smallest rms, ties to the lowest item; no early exit.  The four waves
 * stride over the items; inside an item lanes are columns.  A pair with at most MI_SM_SMALL_ATOMS atoms runs on a smaller LDS tile; both
 * tiles give the same bits.  No atomics, no scratch, no matrix pipe.
 *
 * Pair status: MI_SM_OK; MI_SM_NO_LATTICE (no map: rms = max_dist = +inf); MI_SM_BOX_CAP (more than MI_SM_BOX_POINTS box points, or more
 * than MI_SM_MAX_CAND candidate vectors for an axis); MI_SM_MAP_CAP (more than MI_SM_MAX_MAPS maps); MI_SM_SPECIES_MISMATCH;
 * MI_SM_BAD_PAIR (an index outside its set); MI_SM_NOT_PREPARED (a crystal whose prepare status is not OK).  Every status but OK gives
 * rms = max_dist = +inf, best_map 0, best_trans -1, the counts found so far and perm -1.
 */
#ifndef MATINVENT_HIP_SMATCH_H
#define MATINVENT_HIP_SMATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_SM_MAX_ATOMS 64
#define MI_SM_SMALL_ATOMS 32
#define MI_SM_MAX_SPECIES 16
#define MI_SM_MAX_MAPS 256
#define MI_SM_MAX_CAND 128
#define MI_SM_BOX_POINTS 32768
#define MI_SM_MIN_VOLUME 0.1

#define MI_SM_PREP_OK 0
#define MI_SM_PREP_BAD_INPUT 1
#define MI_SM_PREP_TOO_MANY_ATOMS 2
#define MI_SM_PREP_TOO_MANY_SPECIES 3
#define MI_SM_PREP_DEGENERATE_CELL 4
#define MI_SM_PREP_REDUCE_CAP 5

#define MI_SM_OK 0
#define MI_SM_NO_LATTICE 1
#define MI_SM_BOX_CAP 2
#define MI_SM_MAP_CAP 3
#define MI_SM_SPECIES_MISMATCH 4
#define MI_SM_BAD_PAIR 5
#define MI_SM_NOT_PREPARED 6

/* a prepared set of B crystals with N atoms in all */
typedef struct mi_sm_prepared {
    const int* offsets;  /* [B + 1]: the caller's */
    double* lat;         /* [B][9]: reduced, unit volume per atom */
    double* inv;         /* [B][9]: its inverse */
    double* frac;        /* [N][3]: reduced basis, [0, 1), sorted by species */
    int* types;          /* [N]: sorted atomic numbers */
    int* perm;           /* [N]: sorted position -> the caller's index inside the crystal */
    int* spec_Z;         /* [B][16]: the species, ascending; 0 past the last */
    int* spec_off;       /* [B][17]: block starts; the atom count past the last */
    int* info;           /* [B][4]: atoms, species, rarest species' index, status */
    int B, N;
} mi_sm_prepared;

typedef struct mi_sm_match_args {
    mi_sm_prepared a, b; /* the query set and the candidate set (may be the same) */
    const int* pair_q;   /* [P] rows of a */
    const int* pair_c;   /* [P] rows of b */
    double* rms;         /* [P] */
    double* max_dist;    /* [P] */
    int* best_map;       /* [P][9] */
    int* best_trans;     /* [P] */
    int* n_maps;         /* [P] */
    int* n_items;        /* [P] */
    int* status;         /* [P] */
    int* perm;           /* [P][64] or null: query atom (caller's index) -> candidate atom (caller's index); -1 past the atoms */
    int* maps;           /* [P][MI_SM_MAX_MAPS][9] or null: the map list in order (tests) */
    double ltol, cos_tol;
    int P;
    int large_tile;      /* debug: non-zero runs every pair on the 64-atom tile */
} mi_sm_match_args;

/* mi_sm_prepare: one launch on `stream`.  MI_EINVAL before anything is enqueued: a null pointer, a negative count.  B == 0: MI_OK without
 * a launch.  `types`, `frac` [N][3], `lat` [B][9] are the caller's float32 / int32 arrays. */
int mi_sm_prepare(const int* types, const float* frac, const float* lat, const mi_sm_prepared* out, void* stream);

/* mi_sm_match: two launches on `stream` (the two tile sizes; a workgroup whose pair belongs to the other leaves at once).  MI_EINVAL: a
 * null pointer, a negative count, ltol outside [0, 1), cos_tol outside (0, 1].  P == 0: MI_OK without a launch. */
int mi_sm_match(const mi_sm_match_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif
