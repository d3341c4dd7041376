/*
 * matinvent_hip_stride.h -- strided reverse chains: a batch handle's map from the STEP INDEX k of a chain on S of the T trained steps to
 * the trained time tau_k (DiffCSPModule.respaced).  Same conventions as matinvent_hip.h (device pointers unless a name ends in
 * `_host`, int32 indices, 0 or a negative MI_E* code); a header of its own because the entry lists of the other headers are fixed.
 *
 * A strided chain runs the kernels of the full chain.  Its coefficient table has S + 1 rows, its record buffers S + 1 slots and its
 * counter-based noise the step field k: all of them are indexed by the step index, which is what the `t` / `T` / `t_start` / `t_stop`
 * arguments of mi_sampler_run, mi_traj_logprob, mi_traj_pg_step and mi_traj_pg_kl_step then mean.  The ONE thing that needs the trained
 * time is the time embedding fed to the network, and the map supplies it.
 */
#ifndef MATINVENT_HIP_STRIDE_H
#define MATINVENT_HIP_STRIDE_H

#include "matinvent_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mi_batch_set_time_map: attach map_host[0 .. n-1] (tau_0 .. tau_S, n = S + 1 >= 2) to the handle, or clear it with n = 0 (map_host may
 * then be NULL).  The map must start at 0 and be strictly increasing (MI_EINVAL otherwise; the handle keeps what it had).  It is copied to
 * the device HERE, with a blocking copy -- never inside a chain; set it while no work of this handle is in flight (in practice: right after
 * the handle is created).
 *
 * With a map, three places embed map[k] where they embedded k, through a kernel of their own (one thread per output element, the same
 * float arithmetic as the unmapped kernel, so an identity map gives the same bits):
 *   mi_sampler_run                          every step's embedding (scalar k);
 *   mi_traj_logprob / mi_traj_pg_step       the per-crystal embedding of the evaluation pair -- the map of b_corr, which b_pred must share;
 *   mi_traj_pg_kl_step                      also the prior's embedding -- the map of b_prior.
 * A handle without a map makes exactly the calls it made before this header existed.
 *
 * Refused with MI_EINVAL by those entries before anything is enqueued: a map whose length is not the call's T + 1; b_corr and b_pred with
 * different maps (one with, one without included); in the KL step a b_prior whose map differs from b_corr's. */
int mi_batch_set_time_map(mi_batch* b, const int* map_host, int n);

#ifdef __cplusplus
}
#endif

#endif
