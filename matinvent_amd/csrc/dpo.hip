// The preference (Diffusion-DPO) fine-tune micro-step (include/matinvent_hip_dpo.h): a batch handle's pair lists and the loss
// stage that mi_dpo_micro_step passes to the fine-tune micro-step's driver (backward.hip: ft_micro_run).  Three launches, no atomics:
//   dpo_delta_kernel  one block per crystal: d_b in the factorised form, L_b(agent);
//   dpo_pair_kernel   one block: m_p, g_p of every pair and the three statistics sums;
//   dpo_seed_kernel   one block per crystal: its pairs' signed g_p summed in ascending pair index, the three seed arrays.
#include "../../include/matinvent_hip_dpo.h"
#include "net.h"

namespace mi {

// (sum over the block's 256 threads, the same tree for every call: xor butterfly inside a wave, then (w0 + w1) + (w2 + w3))
__device__ __forceinline__ float dpo_block_sum(float v, float* red, int tid) {
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

struct DpoDeltaArgs {
    const float *pl, *px, *pt, *plp, *pxp, *ptp, *rl, *tx, *rt;
    const int* node_off;
    float *delta, *Lb;
    float cl, cx, ct;
};
// d_b = L_b(agent) - L_b(prior) as cl mean9(f) + cx mean_i mean3(f) + ct mean_i mean100(f), f = (pa - pp)(pa + pp - 2 target) per element
// (= (pa - target)^2 - (pp - target)^2 without the cancellation of two sums that agree to many digits), and L_b(agent) with ft_loss_kernel's
// loops.  Everything a block reads is its own crystal's: d_b does not depend on where the crystal sits in the batch.
__global__ __launch_bounds__(256) void dpo_delta_kernel(DpoDeltaArgs a) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n0 = a.node_off[b], n1 = a.node_off[b + 1], n = n1 - n0;
    const float inv_n = n > 0 ? 1.0f / (float)n : 0.f;
    float sl = 0.f, fl = 0.f;
    if (tid < 9) {
        const int i = b * 9 + tid;
        const float pa = a.pl[i], pp = a.plp[i], tg = a.rl[i], e = pa - tg;
        sl = e * e;
        fl = (pa - pp) * (pa + pp - 2.0f * tg);
    }
    float sx = 0.f, fx = 0.f;
    for (int i = n0 * 3 + tid; i < n1 * 3; i += 256) {
        const float pa = a.px[i], pp = a.pxp[i], tg = a.tx[i], e = pa - tg;
        sx += e * e;
        fx += (pa - pp) * (pa + pp - 2.0f * tg);
    }
    float st = 0.f, ft = 0.f;
    for (int64_t i = (int64_t)n0 * MI_NUM_TYPES + tid; i < (int64_t)n1 * MI_NUM_TYPES; i += 256) {
        const float pa = a.pt[i], pp = a.ptp[i], tg = a.rt[i], e = pa - tg;
        st += e * e;
        ft += (pa - pp) * (pa + pp - 2.0f * tg);
    }
    sl = dpo_block_sum(sl, red, tid); fl = dpo_block_sum(fl, red, tid);
    sx = dpo_block_sum(sx, red, tid); fx = dpo_block_sum(fx, red, tid);
    st = dpo_block_sum(st, red, tid); ft = dpo_block_sum(ft, red, tid);
    if (tid == 0) {
        a.Lb[b] = a.cl * sl / 9.0f + a.cx * sx * inv_n / 3.0f + a.ct * st * inv_n / (float)MI_NUM_TYPES;
        a.delta[b] = a.cl * fl / 9.0f + a.cx * fx * inv_n / 3.0f + a.ct * ft * inv_n / (float)MI_NUM_TYPES;
    }
}

// softplus(u) = max(u, 0) + log1p(exp(-|u|)) and sigmoid(u) on the branch whose exponential cannot overflow
__device__ __forceinline__ float dpo_softplus(float u) { return fmaxf(u, 0.f) + log1pf(expf(-fabsf(u))); }
__device__ __forceinline__ float dpo_sigmoid(float u) {
    const float e = expf(-fabsf(u));
    return u >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}

// One block: m_p = d_w - d_l, g_p = sigmoid(beta m_p) of every pair; thread i sums loss_p, [m_p < 0] and -m_p over p = i, i + 256, ... in
// that order, the block sums the threads with the fixed tree; stats += (or nothing: stats == NULL).
__global__ __launch_bounds__(256) void dpo_pair_kernel(const float* __restrict__ delta, const int* __restrict__ w, const int* __restrict__ l, int P,
                                                       float beta, float inv_pglobal, float* __restrict__ m_out, float* __restrict__ g_out,
                                                       float* __restrict__ stats) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    float s_loss = 0.f, s_neg = 0.f, s_m = 0.f;
    for (int p = tid; p < P; p += 256) {
        const float m = delta[w[p]] - delta[l[p]], u = beta * m;
        m_out[p] = m;
        g_out[p] = dpo_sigmoid(u);
        s_loss += dpo_softplus(u);
        s_neg += m < 0.f ? 1.0f : 0.f;
        s_m += -m;
    }
    s_loss = dpo_block_sum(s_loss, red, tid);
    s_neg = dpo_block_sum(s_neg, red, tid);
    s_m = dpo_block_sum(s_m, red, tid);
    if (tid == 0 && stats) {
        stats[0] += s_loss * inv_pglobal;
        stats[1] += s_neg;
        stats[2] += s_m;
    }
}

struct DpoSeedArgs {
    const float *pl, *px, *pt, *rl, *tx, *rt, *g;
    const int *node_off, *slot_off, *slots;
    float *dl, *dx, *dt;
    float cl, cx, ct, scale;   // scale = inv_denom beta
};
// One block per crystal: c_b = scale (sum of g_p over the pairs it wins - sum over the pairs it loses) -- thread i takes the crystal's slots
// i, i + 256, ... (ascending pair index), the block sums the threads with the fixed tree -- and the seeds c_b cl 2 (pl - rl) / 9, ...
// A crystal in no pair: zeros are stored, whatever its predictions hold.
__global__ __launch_bounds__(256) void dpo_seed_kernel(DpoSeedArgs a) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n0 = a.node_off[b], n1 = a.node_off[b + 1], n = n1 - n0;
    const int k0 = a.slot_off[b], k1 = a.slot_off[b + 1];
    const bool paired = k1 > k0;   // (uniform over the block)
    float sg = 0.f;
    for (int k = k0 + tid; k < k1; k += 256) {
        const int e = a.slots[k];
        const float g = a.g[e >> 1];
        sg += (e & 1) ? -g : g;
    }
    const float c = a.scale * dpo_block_sum(sg, red, tid);
    const float inv_n = n > 0 ? 1.0f / (float)n : 0.f;
    if (tid < 9) {
        const int i = b * 9 + tid;
        a.dl[i] = paired ? (c * a.cl * 2.0f * (a.pl[i] - a.rl[i])) / 9.0f : 0.f;
    }
    for (int i = n0 * 3 + tid; i < n1 * 3; i += 256)
        a.dx[i] = paired ? (c * a.cx * 2.0f * (a.px[i] - a.tx[i])) * inv_n / 3.0f : 0.f;
    for (int64_t i = (int64_t)n0 * MI_NUM_TYPES + tid; i < (int64_t)n1 * MI_NUM_TYPES; i += 256)
        a.dt[i] = paired ? (c * a.ct * 2.0f * (a.pt[i] - a.rt[i])) * inv_n / (float)MI_NUM_TYPES : 0.f;
}

struct DpoStage {
    mi_batch* ab;
    float beta;
    int p_global;
    float *stats, *out_delta, *out_margin;
};
static int dpo_stage(const FtStageIO& io, void* ctx, hipStream_t s) {
    const DpoStage& c = *(const DpoStage*)ctx;
    const mi_batch* ab = c.ab;
    const int B = io.B, P = ab->n_pairs;
    DpoDeltaArgs da{io.pl, io.px, io.pt, io.plp, io.pxp, io.ptp, io.rl, io.tx, io.rt, io.node_off, ab->dpo_delta, io.Lb, io.cl, io.cx, io.ct};
    hipLaunchKernelGGL(dpo_delta_kernel, dim3(B), dim3(256), 0, s, da);
    hipLaunchKernelGGL(dpo_pair_kernel, dim3(1), dim3(256), 0, s, ab->dpo_delta, ab->dpo_w, ab->dpo_l, P, c.beta, 1.0f / (float)c.p_global,
                       ab->dpo_m, ab->dpo_g, c.stats);
    DpoSeedArgs sa{io.pl, io.px, io.pt, io.rl, io.tx, io.rt, ab->dpo_g, io.node_off, ab->dpo_off, ab->dpo_slots, io.dl, io.dx, io.dt,
                   io.cl, io.cx, io.ct, c.beta / ((float)c.p_global * (float)io.accum_steps)};
    hipLaunchKernelGGL(dpo_seed_kernel, dim3(B), dim3(256), 0, s, sa);
    MI_KERNEL_CHECK();
    if (c.out_delta) MI_HIP(hipMemcpyAsync(c.out_delta, ab->dpo_delta, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    if (c.out_margin) MI_HIP(hipMemcpyAsync(c.out_margin, ab->dpo_m, (size_t)P * 4, hipMemcpyDeviceToDevice, s));
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_batch_set_pairs(mi_batch* b, const int* winners_host, const int* losers_host, int n_pairs) {
    MI_NO_POOLED(b, "mi_batch_set_pairs");
    MI_CHECK(b, MI_EINVAL, "null handle");
    MI_CHECK(n_pairs >= 0, MI_EINVAL, "n_pairs = %d: must be >= 0", n_pairs);
    if (n_pairs == 0) {
        b->n_pairs = 0;
        b->dpo_w_h.clear();
        b->dpo_l_h.clear();
        return MI_OK;
    }
    MI_CHECK(winners_host && losers_host, MI_EINVAL, "null pair array");
    const int B = b->B, P = n_pairs;
    MI_CHECK(P <= (1 << 29), MI_EINVAL, "n_pairs = %d: too many", P);
    for (int p = 0; p < P; ++p) {
        const int w = winners_host[p], l = losers_host[p];
        MI_CHECK(w >= 0 && w < B && l >= 0 && l < B, MI_EINVAL, "pair %d = (%d, %d): a crystal index outside [0, %d)", p, w, l, B);
        MI_CHECK(w != l, MI_EINVAL, "pair %d = (%d, %d): winner and loser are the same crystal", p, w, l);
    }
    // per crystal, the slots 2 p (winner) / 2 p + 1 (loser) it sits in, ascending in p: a counting sort by crystal
    std::vector<int> off((size_t)B + 1, 0), slots((size_t)2 * P);
    for (int p = 0; p < P; ++p) {
        ++off[winners_host[p] + 1];
        ++off[losers_host[p] + 1];
    }
    for (int c = 0; c < B; ++c) off[c + 1] += off[c];
    std::vector<int> cur(off.begin(), off.end() - 1);
    for (int p = 0; p < P; ++p) {
        slots[cur[winners_host[p]]++] = 2 * p;
        slots[cur[losers_host[p]]++] = 2 * p + 1;
    }
    if (P > b->pairs_cap) {
        int *w = nullptr, *l = nullptr, *sl = nullptr;
        float *m = nullptr, *g = nullptr;
        MI_TRY(dev_alloc(b, &w, (size_t)P));
        MI_TRY(dev_alloc(b, &l, (size_t)P));
        MI_TRY(dev_alloc(b, &sl, (size_t)2 * P));
        MI_TRY(dev_alloc(b, &m, (size_t)P));
        MI_TRY(dev_alloc(b, &g, (size_t)P));
        b->dpo_w = w, b->dpo_l = l, b->dpo_slots = sl, b->dpo_m = m, b->dpo_g = g;
        b->pairs_cap = P;
    }
    if (!b->dpo_off) {
        MI_TRY(dev_alloc(b, &b->dpo_off, (size_t)B + 1));
        MI_TRY(dev_alloc(b, &b->dpo_delta, (size_t)B));
    }
    MI_HIP(hipMemcpy(b->dpo_w, winners_host, (size_t)P * sizeof(int), hipMemcpyHostToDevice));
    MI_HIP(hipMemcpy(b->dpo_l, losers_host, (size_t)P * sizeof(int), hipMemcpyHostToDevice));
    MI_HIP(hipMemcpy(b->dpo_slots, slots.data(), (size_t)2 * P * sizeof(int), hipMemcpyHostToDevice));
    MI_HIP(hipMemcpy(b->dpo_off, off.data(), ((size_t)B + 1) * sizeof(int), hipMemcpyHostToDevice));
    b->n_pairs = P;
    b->dpo_w_h.assign(winners_host, winners_host + P);
    b->dpo_l_h.assign(losers_host, losers_host + P);
    return MI_OK;
}

int mi_batch_num_pairs(const mi_batch* b) { return b ? b->n_pairs : 0; }

int mi_dpo_micro_step(mi_net* agent, mi_batch* ab, mi_net* prior, mi_batch* pb, const float* lengths, const float* angles,
                      const float* frac0, const int* atom_types, const float* time_freqs, int t, float c0, float c1, float sigma_t,
                      float sigma_norm, uint64_t seed, uint32_t noise_step, const float* rand_l, const float* rand_x, const float* rand_t,
                      float cost_lattice, float cost_coord, float cost_type, float beta, int p_global, int accum_steps, float* grad_theta,
                      float* stats, float* out_delta, float* out_margin, void* stream, void* aux_stream) {
    MI_NO_LATENT(agent, "mi_dpo_micro_step");
    MI_NO_LATENT(prior, "mi_dpo_micro_step");
    MI_NO_POOLED(ab, "mi_dpo_micro_step");
    MI_NO_POOLED(pb, "mi_dpo_micro_step");
    MI_CHECK(ab, MI_EINVAL, "null argument");
    MI_CHECK(ab->n_pairs >= 1, MI_ESTATE, "the agent's batch handle carries no pairs (mi_batch_set_pairs)");
    MI_CHECK(p_global >= ab->n_pairs, MI_EINVAL, "p_global = %d is below the handle's %d pairs", p_global, ab->n_pairs);
    MI_CHECK(beta == beta, MI_EINVAL, "beta is NaN");
    DpoStage st{ab, beta, p_global, stats, out_delta, out_margin};
    return ft_micro_run("mi_dpo_micro_step", agent, ab, prior, pb, lengths, angles, frac0, atom_types, time_freqs, t, c0, c1, sigma_t, sigma_norm,
                        0, nullptr, nullptr, nullptr, nullptr, nullptr, seed, noise_step, rand_l, rand_x, rand_t, cost_lattice, cost_coord,
                        cost_type, accum_steps, grad_theta, dpo_stage, &st, stream, aux_stream);
}

}  // extern "C"
