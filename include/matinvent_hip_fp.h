/*
 * matinvent_hip_fp.h -- a structure fingerprint per crystal (Oganov & Valle, J. Chem. Phys. 130, 104504 (2009), species-resolved;
 * DESIGN 32): the key of the structure-resolved long-term memory and replay buffer.  Same conventions as matinvent_hip.h (device
 * pointers, int32 indices, 0 or a negative MI_E* code); a header of its own because the entry lists of the other headers are fixed.
 *
 * For a crystal of n atoms with lattice rows L, V = |det L|, its distinct species sorted by atomic number A_1 < ... < A_m and the blocks
 * (a <= b) in row-major order of that sort (block index a m - a (a - 1) / 2 + b - a), bin k of nbins has the centre
 * R_k = (k + 1/2) D, D = r_max / nbins, and
 *     F_ab(k) = C_ab(k) / (4 pi R_k^2 D N_a N_b / V) - 1
 * where C_ab(k) sums, over the ordered pairs (i in A_a, j in A_b) and every lattice translation T with (i, j, T) != (i, i, 0), the
 * Gaussian mass of R = |(x_j - x_i) L + T| that falls into the bin:
 *     1/2 [erf((R_k + D/2 - R) / (sigma sqrt 2)) - erf((R_k - D/2 - R) / (sigma sqrt 2))].
 * The output row is the unit vector u = sqrt(w_ab) F_ab / ||.||, w_ab = N_a N_b / n^2, doubled for a < b (such a block is stored once
 * and stands for two).  Two crystals of one species set are then at the distance d = (1 - u1 . u2) / 2.
 *
 * A contribution is dropped from the bins that lie further than MI_FP_CUT sigma from R: less than erfc(MI_FP_CUT / sqrt 2) / 2 of one count
 * per side.  The translations cover every T that can bring a pair within r_max + MI_FP_CUT sigma: the reach along an axis comes from the
 * cell's perpendicular height V / |b x c| (and cyclic), not from its edge length.  The histogram is accumulated in 2^-32 fixed point
 * with integer additions, which commute: a crystal's row does not depend on its place in the batch, on the batch, or on the run.
 */
#ifndef MATINVENT_HIP_FP_H
#define MATINVENT_HIP_FP_H

#include "matinvent_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_FP_MAX_SPECIES 8
#define MI_FP_MAX_BLOCKS 36 /* MI_FP_MAX_SPECIES (MI_FP_MAX_SPECIES + 1) / 2 */
#define MI_FP_MAX_BINS 64
#define MI_FP_MAX_REACH 16  /* translations per axis: -reach .. reach */
#define MI_FP_CUT 6.0f      /* a contribution's tail is dropped beyond this many sigma */
#define MI_FP_MIN_VOLUME 0.1f /* the geometric filter's volume threshold, A^3 */

/* the status in info[1]; anything but MI_FP_OK comes with a zero row (and the counts that were established before the verdict) */
#define MI_FP_OK 0
#define MI_FP_SPECIES 1   /* more than MI_FP_MAX_SPECIES distinct species */
#define MI_FP_NONFINITE 2 /* a non-finite lattice entry or coordinate (or a norm that is not a positive finite number) */
#define MI_FP_VOLUME 3    /* |det L| below MI_FP_MIN_VOLUME */
#define MI_FP_REACH 4     /* a collapsed cell: more than MI_FP_MAX_REACH translations along an axis */
#define MI_FP_ATOMS 5     /* no atoms, or an atom type outside 1..100 */
/* several at once: ATOMS, then NONFINITE, VOLUME, REACH, SPECIES -- the first that applies */

typedef struct mi_fp_params {
    float r_max; /* A; > 0 */
    float sigma; /* A; > 0 */
    int nbins;   /* 1 .. MI_FP_MAX_BINS */
} mi_fp_params;

/* mi_structure_fingerprint_offsets: crystal b owns the atoms node_off[b] .. node_off[b + 1] - 1 of atom_types [N] (int32 atomic numbers)
 * and frac [N][3]; lattices [B][9], rows = cell vectors.  out_fp [B][MI_FP_MAX_BLOCKS * nbins]: the unit row, blocks past the crystal's
 * own are zero.  out_info [B][4] = (species count, status, the norm before normalisation, translations visited per pair).  One launch,
 * one 256-thread block per crystal; nothing is read back.  MI_EINVAL: a null pointer, B < 0, or params outside the ranges above. */
int mi_structure_fingerprint_offsets(const int* node_off, int B, const int* atom_types, const float* frac, const float* lattices,
                                     const mi_fp_params* params, float* out_fp, float* out_info, void* stream);

/* the same for the crystals of a batch handle */
int mi_structure_fingerprint(const mi_batch* b, const int* atom_types, const float* frac, const float* lattices, const mi_fp_params* params,
                             float* out_fp, float* out_info, void* stream);

#ifdef __cplusplus
}
#endif

#endif
