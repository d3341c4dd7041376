// Log-probabilities of one recorded reverse-diffusion step under the current weights, and their gradient seeds:
// DiffCSPModule.forward_logprb (models/diffcsp/diffusion.py:158-227), include/matinvent_hip_traj.h.
//
// The network evaluations are the library's own (mi_cspnet_forward / _train, mi_cspnet_backward); this unit adds the arithmetic after
// them -- one launch that turns the two evaluations' outputs into the three per-crystal log-probabilities (and, for a taped call, their
// local derivatives with respect to every network output), and one launch that scales those derivatives by the upstream gradients.
// The log-probability terms are the sampler's (logprob.h); the arithmetic mirrors the reference's separately-rounded fp32 tensor ops,
// so contraction into FMAs is disabled for this translation unit, as for sampler.hip.
#pragma clang fp contract(off)

#include <algorithm>
#include <vector>

#include "../../include/matinvent_hip_traj.h"
#include "net.h"
#include "logprob.h"

namespace mi {

struct TrajArgs {
    const int* t;        // [B] diffusion time of each crystal
    const float* coef;   // [T+1][MI_NCOEF]
    const int* node_off; // [B+1]
    const float *x, *x_mid, *l, *a, *x_next, *l_next, *a_next;   // recorded state at t and t-1
    const float *px_corr, *pl, *px_pred, *pt;                      // corrector coordinate head; predictor's three heads
    float* lp;                                                     // [3][B]
    float *dx_corr, *dx_pred, *dl, *dt;                            // local derivatives (taped call) or NULL
    int B;
};

__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum(v);
    int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// one 256-thread block per crystal; every sum runs over a fixed thread-to-element map and a fixed tree: no atomics, same bits every call
__global__ __launch_bounds__(256) void traj_logprob_kernel(TrajArgs a) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const StepCoef c = load_coef(a.coef, a.t[b]);
    const int n0 = a.node_off[b], n1 = a.node_off[b + 1], n = n1 - n0;
    const float cnt = (float)(n > 0 ? n : 1);
    const bool tape = a.dx_corr != nullptr;

    // corrector (diffusion.py:175-192): mu = (x - step_corr * sqrt(sn) * pred_x_corr) % 1, log_prob_wn(x_mid, mu, std_corr)
    // predictor (:194-213):            mu = (x_mid - step_pred * sqrt(sn) * pred_x_pred) % 1, log_prob_wn(x_next, mu, std_pred)
    // d mu / d pred = -step * sqrt(sn) (the `% 1` passes the gradient through unchanged, as in torch); each coordinate enters its crystal's mean
    // with weight 1 / (3 n)
    const float kc = -(c.step_corr * c.sqrt_sn) / 3.0f / cnt, kp = -(c.step_pred * c.sqrt_sn) / 3.0f / cnt;
    float lpc = 0.f, lpp = 0.f;
    for (int idx = n0 * 3 + tid; idx < n1 * 3; idx += 256) {
        float px = a.px_corr[idx] * c.sqrt_sn;
        float mu = pymod1(a.x[idx] - c.step_corr * px);
        float xm = a.x_mid[idx];
        if (tape) {
            float dmu;
            lpc += log_prob_wn_dmu(xm, mu, c.std_corr_sq, &dmu);
            a.dx_corr[idx] = dmu * kc;
        } else {
            lpc += log_prob_wn(xm, mu, c.std_corr_sq);
        }
        px = a.px_pred[idx] * c.sqrt_sn;
        mu = pymod1(xm - c.step_pred * px);
        if (tape) {
            float dmu;
            lpp += log_prob_wn_dmu(a.x_next[idx], mu, c.std_pred_sq, &dmu);
            a.dx_pred[idx] = dmu * kp;
        } else {
            lpp += log_prob_wn(a.x_next[idx], mu, c.std_pred_sq);
        }
    }
    lpc = block_sum_256(lpc, red);
    lpp = block_sum_256(lpp, red);

    // lattice (:215-218): Normal(c0 (l - c1 pred_l), sigma).log_prob(l_next), mean over the 9 entries; d/d pred_l = (l_next - m) / sigma^2 * (-c0 c1) / 9
    float lpl = 0.f;
    if (tid < 9) {
        const int idx = b * 9 + tid;
        const float m = c.c0 * (a.l[idx] - c.c1 * a.pl[idx]);
        const float v = a.l_next[idx];
        lpl = normal_log_prob(v, m, c.sigma_sq, c.log_sigma);
        if (tape) a.dl[idx] = (v - m) / c.sigma_sq * (-(c.c0 * c.c1)) / 9.0f;
    }
    lpl = block_sum_256(lpl, red);

    // atom-type logits (:216-221): the same Normal, mean over the 100 logits, then over the atoms; one wave per atom
    const int lane = tid & 63, wave = tid >> 6;
    const float kt = -(c.c0 * c.c1) / (float)MI_NUM_TYPES / cnt;
    float lpt = 0.f;
    for (int i = n0 + wave; i < n1; i += 4) {
        float s = 0.f;
        for (int k = lane; k < MI_NUM_TYPES; k += 64) {
            const size_t idx = (size_t)i * MI_NUM_TYPES + k;
            const float m = c.c0 * (a.a[idx] - c.c1 * a.pt[idx]);
            const float v = a.a_next[idx];
            s += normal_log_prob(v, m, c.sigma_sq, c.log_sigma);
            if (tape) a.dt[idx] = (v - m) / c.sigma_sq * kt;
        }
        s = wave_sum(s);
        lpt += s / (float)MI_NUM_TYPES;
    }
    __syncthreads();
    if (lane == 0) red[wave] = lpt;
    __syncthreads();
    if (tid == 0) {
        a.lp[b] = (lpl / 3.0f) / 3.0f;                                      // .mean(-1).mean(-1)
        a.lp[a.B + b] = ((red[0] + red[1]) + (red[2] + red[3])) / cnt;      // scatter mean over the atoms
        a.lp[2 * a.B + b] = (lpc / 3.0f) / cnt + (lpp / 3.0f) / cnt;  // corrector + predictor, each a mean over coordinates and atoms
    }
}

struct SeedArgs {
    const float* g;      // [3][B] upstream gradients of (log_prob_l, log_prob_t, log_prob_x)
    const int* n2g;      // [N]
    const float *dl, *dx_corr, *dx_pred, *dt;                      // local derivatives of the forward
    const float *uc_l, *uc_x, *uc_t;                               // upstream gradients of the returned corrector predictions (or NULL)
    float *sc_l, *sc_x, *sc_t, *sp_l, *sp_x, *sp_t;                // seeds of the corrector's / predictor's backward
    int B, N;
};

// one thread per output element of both evaluations: B*9 + N*3 + N*A for each
__global__ __launch_bounds__(256) void traj_seed_kernel(SeedArgs a) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nl = (int64_t)a.B * 9, nx = (int64_t)a.N * 3, nt = (int64_t)a.N * MI_NUM_TYPES;
    if (i < nl) {
        a.sp_l[i] = a.g[i / 9] * a.dl[i];
        a.sc_l[i] = a.uc_l ? a.uc_l[i] : 0.f;
        return;
    }
    i -= nl;
    if (i < nx) {
        const float gx = a.g[2 * a.B + a.n2g[i / 3]];
        a.sp_x[i] = gx * a.dx_pred[i];
        a.sc_x[i] = gx * a.dx_corr[i] + (a.uc_x ? a.uc_x[i] : 0.f);
        return;
    }
    i -= nx;
    if (i < nt) {
        a.sp_t[i] = a.g[a.B + a.n2g[i / MI_NUM_TYPES]] * a.dt[i];
        a.sc_t[i] = a.uc_t ? a.uc_t[i] : 0.f;
    }
}

static int traj_buffers(mi_batch* b) {
    if (b->tr_dx) return MI_OK;
    const size_t nl = (size_t)b->B * 9, nx = (size_t)b->N * 3, nt = (size_t)b->N * MI_NUM_TYPES;
    MI_TRY(dev_alloc(b, &b->tr_dl, nl));
    MI_TRY(dev_alloc(b, &b->tr_dt, nt));
    MI_TRY(dev_alloc(b, &b->tr_sl, nl));
    MI_TRY(dev_alloc(b, &b->tr_sx, nx));
    MI_TRY(dev_alloc(b, &b->tr_st, nt));
    return dev_alloc(b, &b->tr_dx, nx);   // (last: its presence marks the set complete)
}

static bool same_counts(const mi_batch* p, const mi_batch* q) {
    return p->B == q->B && p->N == q->N && p->num_atoms_h == q->num_atoms_h;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_traj_logprob(mi_net* net, mi_batch* bc, mi_batch* bp, const int* t_dev, const float* coef_dev, int T, const float* time_freqs,
                    const float* atom_types, const float* frac, const float* frac_mid, const float* lattices, const float* next_atom_types,
                    const float* next_frac, const float* next_lattices, float* log_prob, float* pred_corr_l, float* pred_corr_x,
                    float* pred_corr_t, int keep_tape, void* stream) {
    MI_CHECK(net && bc && bp, MI_EINVAL, "null handle");
    MI_CHECK(bc != bp, MI_EINVAL, "the corrector and the predictor evaluation need two distinct batch handles");
    MI_CHECK(bc->H == net->H && bc->L == net->L && bp->H == net->H && bp->L == net->L, MI_EINVAL, "batch was created for a different network");
    MI_CHECK(same_counts(bc, bp), MI_EINVAL, "the two batch handles hold different atom counts");
    MI_CHECK(t_dev && coef_dev && time_freqs && atom_types && frac && frac_mid && lattices && next_atom_types && next_frac && next_lattices &&
                 log_prob, MI_EINVAL, "null argument");
    MI_CHECK(T >= 2, MI_EINVAL, "T = %d: a recorded step needs T >= 2", T);
    hipStream_t s = (hipStream_t)stream;
    const int B = bc->B, N = bc->N;
    bc->tr_partner = nullptr;   // whatever was pending on this pair is about to be overwritten
    if (B == 0) return MI_OK;
    std::vector<int> th(B);
    MI_HIP(hipMemcpyAsync(th.data(), t_dev, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < B; ++i)
        MI_CHECK(th[i] >= 2 && th[i] <= T, MI_EINVAL, "timesteps[%d] = %d: a recorded step has t in 2..T = %d", i, th[i], T);
    if (keep_tape) {
        MI_TRY(traj_buffers(bc));
        MI_TRY(traj_buffers(bp));
    }
    // time embedding of each crystal's t (diffusion.py:161), once for both evaluations
    MI_TRY(mi_time_embedding(t_dev, time_freqs, B, net->TD, bc->temb, stream));
    float* cl = pred_corr_l ? pred_corr_l : bc->pred_l;
    float* cx = pred_corr_x ? pred_corr_x : bc->pred_x;
    float* ct = pred_corr_t ? pred_corr_t : bc->pred_t;
    const bool train = keep_tape != 0;
    if (train) {
        MI_TRY(net_tape_prepare(net, bc));
        MI_TRY(net_tape_prepare(net, bp));
    }
    MI_TRY(net_forward(net, bc, bc->temb, atom_types, frac, lattices, cl, cx, ct, s, train));
    MI_TRY(net_forward(net, bp, bc->temb, atom_types, frac_mid, lattices, bp->pred_l, bp->pred_x, bp->pred_t, s, train));
    TrajArgs a;
    a.t = t_dev;
    a.coef = coef_dev;
    a.node_off = bc->node_off;
    a.x = frac, a.x_mid = frac_mid, a.l = lattices, a.a = atom_types;
    a.x_next = next_frac, a.l_next = next_lattices, a.a_next = next_atom_types;
    a.px_corr = cx, a.pl = bp->pred_l, a.px_pred = bp->pred_x, a.pt = bp->pred_t;
    a.lp = log_prob;
    a.dx_corr = train ? bc->tr_dx : nullptr;
    a.dx_pred = train ? bp->tr_dx : nullptr;
    a.dl = train ? bp->tr_dl : nullptr;
    a.dt = train ? bp->tr_dt : nullptr;
    a.B = B;
    hipLaunchKernelGGL(traj_logprob_kernel, dim3(B), dim3(256), 0, s, a);
    MI_KERNEL_CHECK();
    if (train && N > 0) {
        bc->tr_partner = bp;
        bc->tr_epoch = bc->fwd_epoch;
        bc->tr_partner_epoch = bp->fwd_epoch;
    }
    return MI_OK;
}

int mi_traj_logprob_backward(mi_net* net, mi_batch* bc, mi_batch* bp, const float* g_logp, const float* d_corr_l, const float* d_corr_x,
                             const float* d_corr_t, float* grad_theta, void* stream) {
    MI_CHECK(net && bc && bp && g_logp && grad_theta, MI_EINVAL, "null argument");
    MI_CHECK(net->W2T != nullptr, MI_ESTATE, "mi_net_set_params must run before backward");
    if (bc->B == 0 || bc->N == 0) return MI_OK;
    MI_CHECK(bc->tr_partner == bp && bc->tr_epoch == bc->fwd_epoch && bp->fwd_epoch == bc->tr_partner_epoch && bc->tape.valid && bp->tape.valid,
             MI_ESTATE, "mi_traj_logprob_backward: no taped mi_traj_logprob pending on these handles (not taped, or a later evaluation overwrote it)");
    hipStream_t s = (hipStream_t)stream;
    const int B = bc->B, N = bc->N;
    SeedArgs a;
    a.g = g_logp;
    a.n2g = bc->node2graph;
    a.dl = bp->tr_dl, a.dx_corr = bc->tr_dx, a.dx_pred = bp->tr_dx, a.dt = bp->tr_dt;
    a.uc_l = d_corr_l, a.uc_x = d_corr_x, a.uc_t = d_corr_t;
    a.sc_l = bc->tr_sl, a.sc_x = bc->tr_sx, a.sc_t = bc->tr_st;
    a.sp_l = bp->tr_sl, a.sp_x = bp->tr_sx, a.sp_t = bp->tr_st;
    a.B = B, a.N = N;
    const int64_t n = (int64_t)B * 9 + (int64_t)N * (3 + MI_NUM_TYPES);
    hipLaunchKernelGGL(traj_seed_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, a);
    MI_KERNEL_CHECK();
    MI_TRY(net_backward(net, bp, bp->tr_sl, bp->tr_sx, bp->tr_st, grad_theta, s));
    return net_backward(net, bc, bc->tr_sl, bc->tr_sx, bc->tr_st, grad_theta, s);
}

}  // extern "C"
