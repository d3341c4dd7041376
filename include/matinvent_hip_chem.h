/*
 * matinvent_hip_chem.h -- composition validity: charge neutrality over the oxidation states of a user-supplied element table,
 * with the Pauling electronegativity ordering test, for a batch of crystals.  Same conventions as matinvent_hip_hull.h (device pointers,
 * int32 indices, 0 or a negative MI_E* code, nothing read back, everything enqueued on the caller's stream); a header of its own because the
 * entry lists of the other headers are fixed.  Every value is an integer.
 *
 * This is the build's own stated rule.  It restates what the reference's `invalid_filter` asks of mattergen's `is_smact_valid`
 * (pipeline/filters/opt_filter.py:51-52 and :179-180); SMACT's and mattergen's texts are absent from this build, so each of the following
 * is [UPSTREAM-UNVERIFIED]: that a single element is valid without a test; that an all-metal composition is valid without a test
 * (`include_alloys`); that the stoichiometry is reduced by its gcd first; that every element takes ONE oxidation state (no mixed valence);
 * that the combinations are capped at 10^7 and a composition beyond the cap is invalid; that the Pauling test is strict, ignores zero
 * states and fails on a missing electronegativity; that more than 8 elements is invalid; the shape of SMACT's oxidation-state files.
 *
 * The table, indexed by atomic number Z = 0 .. MI_CHEM_MAX_Z (row 0 is never read): present[Z]; n_states[Z] in 0 .. MI_CHEM_MAX_STATES;
 * ox[Z][MI_CHEM_MAX_STATES], the ordered oxidation states, each in -127 .. 127; eneg_rank[Z], the dense rank of the Pauling
 * electronegativity among the table's elements (equal values share a rank, -1: missing; the host ranks float64 values, the device compares
 * integers only); is_metal[Z].  A row whose n_states is outside 0 .. MI_CHEM_MAX_STATES counts as not present.
 *
 * A crystal b owns the atoms node_off[b] .. node_off[b + 1] - 1 of atom_types.  Its composition is its distinct elements in ascending Z,
 * E of them, with counts c_e divided by their gcd.  Statuses, decided in this order (valid: ELEMENTAL, ALLOY, ENUMERATED with n_valid > 0):
 *     BAD_INPUT           zero atoms, a type outside 1 .. 118, or offsets that do not lie inside the list (nothing is read through either)
 *     ELEMENTAL           E == 1
 *     TOO_MANY_ELEMENTS   E > MI_CHEM_MAX_ELEMS
 *     UNKNOWN_ELEMENT     an element is not present
 *     ALLOY               include_alloys and every element is_metal
 *     NO_STATES           some list is empty
 *     TOO_MANY_COMBOS     N = prod n_e > max_combos  (N is formed in 64 bits; N == max_combos runs)
 *     ENUMERATED          otherwise
 * Combination i in [0, N) has its digits in mixed radix with the LAST element fastest (itertools.product order).  It is neutral iff
 * sum_e o_e c_e == 0; a neutral one passes iff use_pauling_test is off, or no element of the composition has rank -1 and every pair with
 * o_a > 0 > o_b has rank_a < rank_b strictly (zero states take no part).
 *
 * Outputs per crystal: valid; status; n_elems (E, also when it is beyond 8; 0 for BAD_INPUT); elems[8] and counts[8] (the first 8 in
 * ascending Z, the counts divided by the gcd of ALL of them; 0 past E and for BAD_INPUT); n_combos (N for NO_STATES, TOO_MANY_COMBOS and
 * ENUMERATED, else 0); n_neutral and n_valid over the FULL enumeration (0 unless ENUMERATED); first, the lowest passing index or -1;
 * first_ox[8], its states (0 past E or without one); per atom, atom_ox: the state of its element under `first`, or 0.  A BAD_INPUT crystal
 * whose offsets are bad has no atom rows to write.
 *
 * Work.  Three launches of 256-thread workgroups, no atomics, no scratch, no matrix pipe: a plan (one workgroup per crystal: composition,
 * gcd, status, N and the chunk count ceil(N / MI_CHEM_CHUNK)); the enumeration (a grid fixed on the host from B and max_combos, at most
 * MI_CHEM_MAX_GRID workgroups, each scanning the chunk counts into its own copy of the work-item table and grid-striding over the items
 * (crystal, chunk)); the reduction (one workgroup per crystal folds its items in chunk order and writes every output).
 */
#ifndef MATINVENT_HIP_CHEM_H
#define MATINVENT_HIP_CHEM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_CHEM_MAX_Z 118
#define MI_CHEM_MAX_STATES 32
#define MI_CHEM_MAX_ELEMS 8
#define MI_CHEM_CHUNK 65536
#define MI_CHEM_MAX_GRID 2048
#define MI_CHEM_MAX_BATCH 4096 /* crystals per call: the work-item table of one call sits in LDS */
#define MI_CHEM_DEFAULT_MAX_COMBOS 10000000

#define MI_CHEM_ENUMERATED 0
#define MI_CHEM_ELEMENTAL 1
#define MI_CHEM_ALLOY 2
#define MI_CHEM_BAD_INPUT 3
#define MI_CHEM_TOO_MANY_ELEMENTS 4
#define MI_CHEM_UNKNOWN_ELEMENT 5
#define MI_CHEM_NO_STATES 6
#define MI_CHEM_TOO_MANY_COMBOS 7

typedef struct mi_chem_args {
    /* the element table, rows 0 .. MI_CHEM_MAX_Z */
    const int* present;    /* [119] */
    const int* n_states;   /* [119] */
    const int* ox;         /* [119][32] */
    const int* eneg_rank;  /* [119] */
    const int* is_metal;   /* [119] */
    /* the crystals */
    const int* node_off;   /* [B + 1] */
    const int* atom_types; /* [N] */
    void* workspace;       /* mi_chem_workspace(B, max_combos) bytes, 16-byte aligned */
    /* outputs */
    int* valid;            /* [B] */
    int* status;           /* [B] */
    int* n_elems;          /* [B] */
    int* elems;            /* [B][8] */
    int* counts;           /* [B][8] */
    int64_t* n_combos;     /* [B] */
    int64_t* n_neutral;    /* [B] */
    int64_t* n_valid;      /* [B] */
    int64_t* first;        /* [B] */
    int* first_ox;         /* [B][8] */
    int* atom_ox;          /* [N] */
    int64_t max_combos;    /* 1 .. 32^8 */
    int B, N;
    int use_pauling_test, include_alloys;
} mi_chem_args;

/* bytes of workspace for B crystals under the cap max_combos; MI_EINVAL: B outside 0 .. MI_CHEM_MAX_BATCH, max_combos outside 1 .. 32^8,
 * or more than 2^31 - 1 work items */
int64_t mi_chem_workspace(int B, int64_t max_combos);

/* mi_chem_validity: three launches on `stream`, nothing read back.  MI_EINVAL before anything is enqueued: a null pointer, a negative
 * count, B beyond MI_CHEM_MAX_BATCH, max_combos outside 1 .. 32^8, a workspace that is not 16-byte aligned.  B == 0: MI_OK without a launch. */
int mi_chem_validity(const mi_chem_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif
