/*
 * matinvent_hip_pool.h -- a device-memory pool for batch handles, and a batch handle created in it (pretrain.fit's mini-batches;
 * DESIGN 39).  Same conventions as matinvent_hip.h (device pointers unless a name ends in `_host`, int32 indices, 0 or a negative MI_E*
 * code); a header of its own because the entry lists of the other headers are fixed.
 *
 * A handle of mi_batch_create owns its device buffers: every one is a hipMalloc, the first training step adds the tape, and
 * mi_batch_destroy frees them all.  A POOLED handle keeps the same exact-size buffers and the same layout -- no kernel can tell the two
 * apart -- but the memory behind them is lent by a pool that outlives the handle, its index tables are written by kernels instead of
 * host loops, and all of its set-up is enqueued on the pool's stream: creating and destroying it waits for nothing.
 *
 * ORDER.  A pool belongs to ONE stream.  A block a handle gives back may be lent to the next handle at once, so every use of a pooled
 * handle must be enqueued on the pool's stream (or on a side stream that forked from it and joined it again, which is what the
 * library's own helper streams do).  The entries that take a pooled handle check their `stream` argument against the pool's.
 *
 * Entries that take a pooled handle:  mi_cspnet_forward, mi_cspnet_forward_train, mi_cspnet_backward, mi_batch_set_wgrad_window,
 * mi_cspnet_wgrad_flush, mi_batch_wgrad_pending, mi_pretrain_micro_step (and the mi_add_noise_per_crystal inside it),
 * mi_structure_check, mi_batch_num_nodes, mi_batch_num_edges, mi_batch_node2graph, mi_batch_index_table, mi_batch_destroy.
 * Entries that REFUSE a pooled handle with MI_EINVAL before anything is enqueued (their chains run on worker streams, or they attach
 * state with blocking copies, which the pool's single-stream order does not cover):  mi_sampler_run, mi_sampler_init_state,
 * mi_sampler_set_keep, mi_traj_logprob, mi_traj_logprob_backward, mi_traj_read_derivatives, mi_traj_pg_step, mi_traj_pg_kl_step,
 * mi_ft_micro_step, mi_ft_micro_steps_stacked, mi_dpo_micro_step, mi_batch_set_pairs, mi_batch_set_condition,
 * mi_batch_set_likelihood_mask, mi_condition_apply, mi_batch_set_resampling, mi_resample_jump, mi_batch_set_time_map, mi_add_noise,
 * mi_cspnet_tap, mi_structure_fingerprint.
 */
#ifndef MATINVENT_HIP_POOL_H
#define MATINVENT_HIP_POOL_H

#include "matinvent_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_pool mi_pool;

/* A pool for `stream`; max_bytes <= 0: no cap on the bytes it reserves.  Calls from several threads are serialised by a mutex. */
int mi_pool_create(void* stream, int64_t max_bytes, mi_pool** out);
/* hipFree of every block; MI_ESTATE (and nothing freed) while handles created in the pool are alive.  Waits for the pool's stream. */
int mi_pool_destroy(mi_pool* pool);
/* hipFree of every cached block that no handle holds (waits for the pool's stream first: a cached block may still be read by work in flight). */
int mi_pool_trim(mi_pool* pool);
/* out[0] bytes reserved (in use + cached), [1] bytes in use, [2] hipMalloc calls, [3] requests served from the free list,
 * [4] hipFree calls, [5] live handles, [6] high-water bytes in use, [7] the cap (0: none).  Bytes are those of the size classes. */
int mi_pool_stats(const mi_pool* pool, int64_t out_host[8]);
/* Host only: the size class of a request of `request` bytes.  Up to 1 MiB the next power of two, at least 512; above 1 MiB the next
 * multiple of one eighth of the largest power of two not above the request (waste <= 12.5 %).  request <= 0: 512. */
int64_t mi_pool_block_bytes(int64_t request);
/* Debug aid: with poison on, every block of float or fp16-plane elements is filled with quiet NaN (0x7FC00000 / 0x7E00) on the pool's
 * stream before it is handed out, fresh or recycled.  (Blocks of int / unsigned elements -- index tables, arrival counters -- are handed
 * out ZERO-FILLED whether poison is on or not.) */
int mi_pool_set_poison(mi_pool* pool, int on);

/* mi_batch_create with the memory taken from `pool`: fully connected edge style only (the knn style has no pooled form:
 * mi_batch_create_knn takes no pool, and the host binding refuses a pool for that style with MI_EINVAL).  The host computes three prefix sums over the B crystals; kernels on
 * the pool's stream write the index tables, value for value those of mi_batch_create.  Nothing synchronises.  MI_ENOMEM when the pool's cap
 * would be exceeded even after its cached blocks were freed: nothing stays taken and the pool stays usable.
 * mi_batch_destroy on the handle gives its blocks back to the pool and frees nothing. */
int mi_batch_create_pooled(const mi_net* net, mi_pool* pool, const int* num_atoms_host, int B, int64_t node_offset, int64_t graph_offset,
                           mi_batch** out);

/* One index table of ANY handle copied to the host (synchronises): which = 0 num_atoms [B], 1 node2graph [N], 2 rowptr [N + 1],
 * 3 e_diag [N], 4 src, 5 dst, 6 edge_graph [E each], 7 pair_i, 8 pair_j, 9 pair_e1, 10 pair_e2, 11 pair_graph [Np each], 12 node_off
 * [B + 1], 13 pair_off [B + 1].  Returns the table's length (host_out NULL: the length alone), or MI_EINVAL for an unknown table or
 * cap < length. */
int64_t mi_batch_index_table(const mi_batch* b, int which, int* host_out, int64_t cap);

#ifdef __cplusplus
}
#endif

#endif
