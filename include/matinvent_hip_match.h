/*
 * matinvent_hip_match.h -- fingerprint matching: for groups of query rows, the nearest row of a device-resident bank, the
 * number of bank rows within a tolerance and, on request, every pair distance.  The relation is the one of matinvent_hip_fp.h: two unit
 * rows u, v of one reduced formula are at d = (1 - u . v) / 2.  Same conventions as matinvent_hip.h (device pointers unless a name ends
 * in _host, int32 indices, int64 element offsets, 0 or a negative MI_E* code); a header of its own because the entry lists of the other
 * headers are fixed.
 *
 * Groups.  Group g (one reduced formula) owns the query positions grp_q_off[g] .. grp_q_off[g + 1] - 1 of q_idx (rows of the query
 * matrix [Q][row_stride]), the candidate positions grp_c_off[g] .. grp_c_off[g + 1] - 1 of c_idx (rows of the bank), and
 * ncols = grp_ncols[g], the leading columns that can be non-zero; len = ncols rounded up to a multiple of 4.
 *
 * Bank.  Ragged and compact: row r owns bank_len[r] floats at element offset bank_start[r] of one float32 buffer of bank_floats
 * elements; bank_len[r] is the row's own ncols rounded up to a multiple of 4, the padding is zero, every start is a multiple of 4.
 * A query row is read over the same len columns (row_stride is a multiple of 4; its columns past ncols are zero).
 *
 * The order of one pair's sum (a fixed function of ncols, nothing else).  With len as above, lane l of 64 owns the columns
 * 4 (l + 64 i) + k, i = 0 .. ceil(len / 256) - 1, k = 0 .. 3, that are below len, and adds their products to one fp32 accumulator that
 * starts at 0, by fused multiply-add, i ascending and within i k ascending.  The 64 accumulators are then added in a butterfly: lanes
 * l and l ^ 32, then l ^ 16, 8, 4, 2, 1, one fp32 addition per level.  d = 0.5f * (1.0f - dot).  The longest chain of sequential
 * additions is therefore
 *     L(ncols) = 4 ceil(ceil4(ncols) / 256) + 6        (MI_FP_MATCH_CHAIN),
 * 10 at ncols <= 256 and 42 at the full width of 2304.  No matrix pipe, no atomics: the bits of a pair's d depend on the two rows and
 * ncols only -- not on the pair's place in a tile, the group's size, the order of the candidate list, the batch or the run.
 *
 * Work.  mi_fp_match_plan (host) cuts the groups into work items (a tile of MI_FP_MATCH_TILE queries x a chunk of candidates); one
 * 256-thread workgroup per item stages the tile's query rows in LDS and streams the chunk's bank rows past it (a bank row is read once per
 * tile, 16 bytes per lane), and writes one partial (best, index, count, status) per query; a second small kernel folds each query's
 * partials in chunk order.  Ties: equal distances resolve to the LOWEST BANK INDEX, whatever the order of the list; best_dist is the
 * bitwise d of the pair (query, best_idx).
 *
 * Guard.  A candidate whose index is outside 0 .. M - 1, whose bank_len differs from the group's len, or whose bank_start is negative,
 * not a multiple of 4 or ends past bank_floats is skipped and the query's status set to 1; nothing is read through such an index.  A
 * query index outside 0 .. Q - 1, a group whose len exceeds row_stride or max_ncols rounded up, and an item that does not lie inside its
 * group are skipped in the same way (nothing read, nothing written): the entry marks every partial as unwritten before the launch, and a
 * query whose chunk was never written gets status 1.
 */
#ifndef MATINVENT_HIP_MATCH_H
#define MATINVENT_HIP_MATCH_H

#include <stdint.h>

#include "matinvent_hip_fp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_FP_MATCH_TILE 8   /* query rows staged per work item */
#define MI_FP_MATCH_ITEM_INTS 5 /* (group, first query position, first candidate position, end candidate position, first partial) */
#define MI_FP_MATCH_CHAIN(ncols) (4 * (((((ncols) + 3) / 4) * 4 + 255) / 256) + 6)

typedef struct mi_fp_match_args {
    /* the rows */
    const float* query;        /* [Q][row_stride] */
    const float* bank;         /* [bank_floats] */
    const int64_t* bank_start; /* [M] */
    const int* bank_len;       /* [M] */
    /* the groups (CSR) */
    const int* grp_q_off;      /* [G + 1] */
    const int* q_idx;          /* [nnz_q] */
    const int* grp_c_off;      /* [G + 1] */
    const int* c_idx;          /* [nnz_c] */
    const int* grp_ncols;      /* [G] */
    /* the plan of mi_fp_match_plan, uploaded by the caller */
    const int* items;          /* [n_items][MI_FP_MATCH_ITEM_INTS] */
    const int* grp_part_off;   /* [G + 1] */
    void* workspace;           /* mi_fp_match_workspace(n_partials) bytes, 16-byte aligned */
    /* outputs, per query row */
    float* best_dist;          /* [Q]; +infinity when the group has no (admissible) candidate */
    int* best_idx;             /* [Q]; -1 when the group has no (admissible) candidate */
    int* n_within;             /* [Q]; candidates with d <= tol */
    int* status;               /* [Q]; 0, or 1 if the guard skipped a candidate */
    float* pair_dist;          /* may be null; group g's [nq_g][nc_g] matrix, row-major, at element pair_off[g]; a skipped pair is left as it was */
    const int64_t* pair_off;   /* [G]; may be null when pair_dist is */
    int64_t bank_floats, pair_floats;
    int Q, row_stride, M, G, nnz_q, nnz_c, n_items, n_partials;
    int max_ncols;             /* the largest grp_ncols: sizes the LDS tile */
    float tol;                 /* in [0, 1] */
} mi_fp_match_args;

/* mi_fp_match_plan (host arrays in, host arrays out; no device work): the work items of G groups.  chunk = candidates per item
 * (a multiple of 16), or <= 0 for the library's choice: the largest power of two in 32 .. 1024 that still gives 2048 items, so that one
 * large group fills the chip and many small groups cost one item each.  A group without candidates has no item.  With items_host and
 * grp_part_off_host null only the counts are returned.  Returns the chunk used, or MI_EINVAL (a null offset array, G < 0, offsets that
 * decrease or start below 0, more than 2^31 - 1 items x MI_FP_MATCH_ITEM_INTS or partials). */
int mi_fp_match_plan(const int* grp_q_off_host, const int* grp_c_off_host, int G, int chunk, int* items_host, int* grp_part_off_host,
                     int64_t* n_items, int64_t* n_partials);

/* bytes of scratch memory for n_partials partials (mi_fp_match_plan); negative n_partials: MI_EINVAL */
int64_t mi_fp_match_workspace(int64_t n_partials);

/* mi_fp_match: one fill of the partials' status and two launches on `stream`, nothing read back.  Queries that belong to no group keep what their output rows held.
 * MI_EINVAL before anything is enqueued: a null pointer (pair_dist alone may be null; pair_off only with it), a negative count,
 * tol outside [0, 1] or not finite, row_stride not a multiple of 4, max_ncols outside 1 .. MI_FP_MAX_BLOCKS * MI_FP_MAX_BINS.
 * G == 0, Q == 0 or nnz_q == 0: MI_OK without a launch. */
int mi_fp_match(const mi_fp_match_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif
