// One micro-step of supervised denoising training (include/matinvent_hip_pretrain.h): the per-crystal time gather, the loss
// of torch's F.mse_loss over all elements of the mini-batch with its gradient seeds, and the four statistics.  The noising is
// backward.hip's add_noise_kernel behind mi_add_noise_per_crystal, the network the taped forward and net_backward.  Three launches of
// its own, no atomics:
//   pretrain_time_kernel   one thread per crystal: the clamped time and the crystal's schedule row;
//   pretrain_loss_kernel   one block per crystal: the seeds and the crystal's three sums of squares;
//   pretrain_stats_kernel  one block: the sums over the crystals in a fixed order, the four statistics.
// The loss mirrors separately rounded fp32 tensor ops: no contraction into FMAs in this unit.
#pragma clang fp contract(off)

#include "../../include/matinvent_hip_pretrain.h"
#include "net.h"

namespace mi {

// (sum over the block's 256 threads, the same tree for every call: xor butterfly inside a wave, then (w0 + w1) + (w2 + w3))
__device__ __forceinline__ float pretrain_block_sum(float v, float* red, int tid) {
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// times[c] = clamp(t[c], 1, T) (the host checked these values: the clamp only keeps the read of a stray one inside the table) and
// sched[c] = table[times[c]]: {sqrt(alpha_bar), sqrt(1 - alpha_bar), sigma, sigmas_norm}
__global__ __launch_bounds__(256) void pretrain_time_kernel(const int* __restrict__ t, const float* __restrict__ table, int* __restrict__ times,
                                                            float* __restrict__ sched, int B, int T) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= B) return;
    const int v = t[c], tc = v < 1 ? 1 : (v > T ? T : v);
    times[c] = tc;
#pragma unroll
    for (int k = 0; k < 4; ++k) sched[c * 4 + k] = table[tc * 4 + k];
}

struct PretrainLossArgs {
    const float *pl, *px, *pt, *rl, *tx, *rt;
    const int* node_off;
    float *dl, *dx, *dt;   // the seeds, or all three NULL (forward-only form)
    float* parts;          // [B][3]
    float cl, cx, ct;
    float den_l, den_x, den_t;   // 9 b_global accum_steps, 3 n_global accum_steps, 100 n_global accum_steps
};
// One block per crystal, ft_loss_kernel's thread-to-element maps: thread i < 9 owns lattice element i, the coordinate and type elements
// i, i + 256, ... of the crystal's rows; e = pred - target, seed = (c 2 e) / den, the crystal's sums of e^2 through the fixed tree.
__global__ __launch_bounds__(256) void pretrain_loss_kernel(PretrainLossArgs a) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n0 = a.node_off[b], n1 = a.node_off[b + 1];
    const bool seeds = a.dl != nullptr;   // (uniform over the grid)
    float sl = 0.f;
    if (tid < 9) {
        const int i = b * 9 + tid;
        const float e = a.pl[i] - a.rl[i];
        sl = e * e;
        if (seeds) a.dl[i] = (a.cl * 2.0f * e) / a.den_l;
    }
    float sx = 0.f;
    for (int i = n0 * 3 + tid; i < n1 * 3; i += 256) {
        const float e = a.px[i] - a.tx[i];
        sx += e * e;
        if (seeds) a.dx[i] = (a.cx * 2.0f * e) / a.den_x;
    }
    float st = 0.f;
    for (int64_t i = (int64_t)n0 * MI_NUM_TYPES + tid; i < (int64_t)n1 * MI_NUM_TYPES; i += 256) {
        const float e = a.pt[i] - a.rt[i];
        st += e * e;
        if (seeds) a.dt[i] = (a.ct * 2.0f * e) / a.den_t;
    }
    sl = pretrain_block_sum(sl, red, tid);
    sx = pretrain_block_sum(sx, red, tid);
    st = pretrain_block_sum(st, red, tid);
    if (tid == 0) {
        a.parts[b * 3] = sl;
        a.parts[b * 3 + 1] = sx;
        a.parts[b * 3 + 2] = st;
    }
}

// One block: thread i sums the crystals i, i + 256, ... in that order, the block sums the threads with the fixed tree;
// stats[1..3] += sum / (9 b_global), / (3 n_global), / (100 n_global), stats[0] += their cost-weighted sum
__global__ __launch_bounds__(256) void pretrain_stats_kernel(const float* __restrict__ parts, int B, float cl, float cx, float ct, float den_l,
                                                             float den_x, float den_t, float* __restrict__ stats) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    float sl = 0.f, sx = 0.f, st = 0.f;
    for (int b = tid; b < B; b += 256) {
        sl += parts[b * 3];
        sx += parts[b * 3 + 1];
        st += parts[b * 3 + 2];
    }
    sl = pretrain_block_sum(sl, red, tid);
    sx = pretrain_block_sum(sx, red, tid);
    st = pretrain_block_sum(st, red, tid);
    if (tid == 0) {
        const float ll = sl / den_l, lx = sx / den_x, lt = st / den_t;
        stats[0] += (cl * ll + cx * lx) + ct * lt;
        stats[1] += ll;
        stats[2] += lx;
        stats[3] += lt;
    }
}

// the handle's buffers of this entry, allocated on first use: the schedule rows and the per-crystal sums; and, for the forward-only form
// (which prepares no tape), the noised inputs and the targets that the taped form keeps in the tape
static int pretrain_buffers(mi_batch* b, bool forward_only) {
    if (!b->pt_sched) {
        MI_TRY(dev_alloc(b, &b->pt_sched, (size_t)b->B * 4));
        MI_TRY(dev_alloc(b, &b->pt_parts, (size_t)b->B * 3));
    }
    if (forward_only && !b->pt_noised) {
        const size_t nl = (size_t)b->B * 9, nx = (size_t)b->N * 3, nt = (size_t)b->N * MI_NUM_TYPES;
        MI_TRY(dev_alloc(b, &b->pt_noised, 2 * (nl + nx + nt)));
    }
    return MI_OK;
}

// the body of the two entries (net.h): `what` names the entry in the messages, `stage` fills b->temb from b->times
int pretrain_micro_run(const char* what, mi_net* net, mi_batch* b, const float* lengths, const float* angles, const float* frac0, const int* atom_types,
                       const float* time_freqs, const int* t_host, const int* t_dev, const float* sched_table_dev, int T, uint64_t seed,
                       uint32_t noise_step, const float* rand_l, const float* rand_x, const float* rand_t, float cost_lattice, float cost_coord,
                       float cost_type, int b_global, int n_global, int accum_steps, float* grad_theta, float* stats, float* out_parts,
                       pretrain_embed_stage_fn stage, void* stage_ctx, void* stream) {
    MI_CHECK(!b || !b->pool || pool_stream(b->pool) == (hipStream_t)stream, MI_EINVAL, "%s: a pooled batch handle is used on its pool's stream only", what);
    MI_CHECK(net && b, MI_EINVAL, "null handle");
    MI_CHECK(b->H == net->H && b->L == net->L, MI_EINVAL, "batch was created for a different network");
    MI_CHECK(!b->time_map, MI_EINVAL, "%s: the handle carries a time map (training runs on the trained grid)", what);
    MI_CHECK(!b->cond_on && !b->lik_on, MI_EINVAL, "%s: the handle carries a condition or a likelihood mask", what);
    MI_CHECK(!b->gd_on, MI_EINVAL, "%s: the handle carries guidance (mi_batch_clear_guidance first)", what);
    MI_CHECK(b->tape.wcur == 0, MI_EINVAL, "%s: the handle has pending deferred weight gradients (mi_cspnet_wgrad_flush first)", what);
    MI_CHECK(!grad_theta || b->tape.wslots == 0, MI_EINVAL, "%s: the handle has an open weight-gradient window (mi_batch_set_wgrad_window(.., 0) first)", what);
    const int B = b->B, N = b->N;
    MI_CHECK(T >= 1 && accum_steps >= 1, MI_EINVAL, "T = %d, accum_steps = %d: both must be >= 1", T, accum_steps);
    MI_CHECK(b_global >= B && n_global >= N, MI_EINVAL, "b_global = %d / n_global = %d are below the handle's %d crystals / %d atoms", b_global, n_global, B, N);
    if (B == 0 || N == 0) return MI_OK;
    MI_CHECK(lengths && angles && frac0 && atom_types && time_freqs && t_host && t_dev && sched_table_dev, MI_EINVAL, "null argument");
    for (int c = 0; c < B; ++c) MI_CHECK(t_host[c] >= 1 && t_host[c] <= T, MI_EINVAL, "t[%d] = %d: a training time lies in 1..T = %d", c, t_host[c], T);
    MI_CHECK(!grad_theta || net->W2T != nullptr, MI_ESTATE, "mi_net_set_params must run before backward");
    TraceRange range(what);
    hipStream_t s = (hipStream_t)stream;
    const bool train = grad_theta != nullptr;
    if (train) MI_TRY(net_tape_prepare(net, b));
    MI_TRY(pretrain_buffers(b, !train));
    Tape& tp = b->tape;
    const size_t nl = (size_t)B * 9, nx = (size_t)N * 3, nt = (size_t)N * MI_NUM_TYPES;
    float* const q = b->pt_noised;   // (forward-only: in_lat | in_frac | in_types | tar_x | rnd_l | rnd_t)
    float* const nz_lat = train ? tp.nz_lat : q;
    float* const nz_frac = train ? tp.nz_frac : q + nl;
    float* const nz_types = train ? tp.nz_types : q + nl + nx;
    float* const tar_x = train ? tp.tar_x : q + nl + nx + nt;
    float* const rnd_l = train ? tp.rnd_l : q + nl + 2 * nx + nt;
    float* const rnd_t = train ? tp.rnd_t : q + 2 * nl + 2 * nx + nt;

    hipLaunchKernelGGL(pretrain_time_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, t_dev, sched_table_dev, b->times, b->pt_sched, B, T);
    MI_KERNEL_CHECK();
    MI_TRY(stage(net, b, time_freqs, stage_ctx, s));
    MI_TRY(mi_add_noise_per_crystal(b, lengths, angles, frac0, atom_types, b->pt_sched, seed, noise_step, rand_l, rand_x, rand_t, nz_lat, nz_frac,
                                    nz_types, tar_x, rnd_l, rnd_t, stream));
    if (train) {
        tp.borrow_inputs = true;   // (the noised inputs live in this tape and the time embedding in this batch until the backward below has run)
        const int rc = net_forward(net, b, b->temb, nz_types, nz_frac, nz_lat, b->pred_l, b->pred_x, b->pred_t, s, true);
        tp.borrow_inputs = false;
        MI_TRY(rc);
    } else {
        MI_TRY(net_forward(net, b, b->temb, nz_types, nz_frac, nz_lat, b->pred_l, b->pred_x, b->pred_t, s, false));
    }
    const double bg = (double)b_global, ng = (double)n_global, ac = (double)accum_steps;
    PretrainLossArgs la{b->pred_l, b->pred_x, b->pred_t, rnd_l, tar_x, rnd_t, b->node_off,
                        train ? tp.d_l : nullptr, train ? tp.d_x : nullptr, train ? tp.d_t : nullptr, b->pt_parts,
                        cost_lattice, cost_coord, cost_type, (float)(9.0 * bg * ac), (float)(3.0 * ng * ac), (float)((double)MI_NUM_TYPES * ng * ac)};
    hipLaunchKernelGGL(pretrain_loss_kernel, dim3(B), dim3(256), 0, s, la);
    if (stats)
        hipLaunchKernelGGL(pretrain_stats_kernel, dim3(1), dim3(256), 0, s, b->pt_parts, B, cost_lattice, cost_coord, cost_type, (float)(9.0 * bg),
                           (float)(3.0 * ng), (float)((double)MI_NUM_TYPES * ng), stats);
    MI_KERNEL_CHECK();
    if (out_parts) MI_HIP(hipMemcpyAsync(out_parts, b->pt_parts, (size_t)B * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (!train) return MI_OK;
    return net_backward(net, b, tp.d_l, tp.d_x, tp.d_t, grad_theta, s);
}

static int pretrain_time_stage(mi_net* net, mi_batch* b, const float* time_freqs, void*, hipStream_t s) {
    return mi_time_embedding(b->times, time_freqs, b->B, net->TD, b->temb, s);
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_pretrain_micro_step(mi_net* net, mi_batch* b, const float* lengths, const float* angles, const float* frac0, const int* atom_types,
                           const float* time_freqs, const int* t_host, const int* t_dev, const float* sched_table_dev, int T, uint64_t seed,
                           uint32_t noise_step, const float* rand_l, const float* rand_x, const float* rand_t, float cost_lattice,
                           float cost_coord, float cost_type, int b_global, int n_global, int accum_steps, float* grad_theta, float* stats,
                           float* out_parts, void* stream) {
    MI_NO_LATENT(net, "mi_pretrain_micro_step");
    return pretrain_micro_run("mi_pretrain_micro_step", net, b, lengths, angles, frac0, atom_types, time_freqs, t_host, t_dev, sched_table_dev, T, seed,
                              noise_step, rand_l, rand_x, rand_t, cost_lattice, cost_coord, cost_type, b_global, n_global, accum_steps, grad_theta, stats,
                              out_parts, pretrain_time_stage, nullptr, stream);
}

}  // extern "C"
