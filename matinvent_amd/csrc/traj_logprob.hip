// Log-probabilities of one recorded reverse-diffusion step under the current weights, and their gradient seeds:
// DiffCSPModule.forward_logprb (models/diffcsp/diffusion.py:158-227), include/matinvent_hip_traj.h; and the policy-gradient micro-step built
// on them, with or without the KL anchor to a frozen prior (include/matinvent_hip_pg.h, _pg_kl.h): its stages are listed at pg_enqueue.
//
// The network evaluations are the library's own (net_forward, net_backward); this unit adds the arithmetic around them.  The log-probability
// terms are the sampler's (logprob.h); the arithmetic mirrors the reference's separately-rounded fp32 tensor ops, so contraction into FMAs is
// disabled for this translation unit, as for sampler.hip.
#pragma clang fp contract(off)

#include <vector>

#include "../../include/matinvent_hip_traj.h"
#include "../../include/matinvent_hip_pg.h"
#include "../../include/matinvent_hip_pg_kl.h"
#include "../../include/matinvent_hip_lik.h"
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

// traj_logprob_kernel under a likelihood mask: the predictor terms of the known elements leave the sums and their local derivatives are
// 0.f; the divisors, the corrector term, the thread-to-element maps, the reduction trees and every free element's arithmetic are
// traj_logprob_kernel's, line for line -- a kernel of its own, so that traj_logprob_kernel's device code stays what it was.
__global__ __launch_bounds__(256) void traj_logprob_masked_kernel(TrajArgs a, LikMask m) {
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
        if (m.known_coords[idx / 3]) {   // the imposition replaced this coordinate: its predictor term is a constant of theta
            if (tape) a.dx_pred[idx] = 0.f;
        } else {
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
    }
    lpc = block_sum_256(lpc, red);
    lpp = block_sum_256(lpp, red);

    // lattice (:215-218): Normal(c0 (l - c1 pred_l), sigma).log_prob(l_next), mean over the 9 entries; d/d pred_l = (l_next - m) / sigma^2 * (-c0 c1) / 9
    float lpl = 0.f;
    if (tid < 9) {
        const int idx = b * 9 + tid;
        if (m.known_lattice[b]) {
            if (tape) a.dl[idx] = 0.f;
        } else {
            const float mean = c.c0 * (a.l[idx] - c.c1 * a.pl[idx]);
            const float v = a.l_next[idx];
            lpl = normal_log_prob(v, mean, c.sigma_sq, c.log_sigma);
            if (tape) a.dl[idx] = (v - mean) / c.sigma_sq * (-(c.c0 * c.c1)) / 9.0f;
        }
    }
    lpl = block_sum_256(lpl, red);

    // atom-type logits (:216-221): the same Normal, mean over the 100 logits, then over the atoms; one wave per atom
    const int lane = tid & 63, wave = tid >> 6;
    const float kt = -(c.c0 * c.c1) / (float)MI_NUM_TYPES / cnt;
    float lpt = 0.f;
    for (int i = n0 + wave; i < n1; i += 4) {
        if (m.known_types[i]) {   // (the same for every lane of the wave: the atom's row leaves the sum whole)
            if (tape)
                for (int k = lane; k < MI_NUM_TYPES; k += 64) a.dt[(size_t)i * MI_NUM_TYPES + k] = 0.f;
            continue;
        }
        float s = 0.f;
        for (int k = lane; k < MI_NUM_TYPES; k += 64) {
            const size_t idx = (size_t)i * MI_NUM_TYPES + k;
            const float mean = c.c0 * (a.a[idx] - c.c1 * a.pt[idx]);
            const float v = a.a_next[idx];
            s += normal_log_prob(v, mean, c.sigma_sq, c.log_sigma);
            if (tape) a.dt[idx] = (v - mean) / c.sigma_sq * kt;
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
    const float *uc_l, *uc_x, *uc_t;                               // !KL: upstream gradients of the returned corrector predictions (or NULL)
    float *sc_l, *sc_x, *sc_t, *sp_l, *sp_x, *sp_t;                // seeds of the corrector's / predictor's backward
    int B, N;
    const float *kdl, *kdxc, *kdxp, *kdt;                          // KL: the KL's local derivatives ...
    float kl0, kl1, kl2;                                           // ... and their weights kl_coef * loss_scale * w_k
};

// one thread per output element of both evaluations: B*9 + N*3 + N*A for each.  !KL: seed = g_b dlp, plus the corrector predictions' own
// upstream gradient (+ 0.f without one).  KL: seed = g_b dlp + (kl_coef loss_scale w_k) dKL; the corrector's lattice and type heads enter
// neither term, their seeds are zero.
template <bool KL>
__global__ __launch_bounds__(256) void traj_seed_kernel(SeedArgs a) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nl = (int64_t)a.B * 9, nx = (int64_t)a.N * 3, nt = (int64_t)a.N * MI_NUM_TYPES;
    if (i < nl) {
        a.sp_l[i] = KL ? a.g[i / 9] * a.dl[i] + a.kl0 * a.kdl[i] : a.g[i / 9] * a.dl[i];
        a.sc_l[i] = !KL && a.uc_l ? a.uc_l[i] : 0.f;
        return;
    }
    i -= nl;
    if (i < nx) {
        const float gx = a.g[2 * a.B + a.n2g[i / 3]];
        a.sp_x[i] = KL ? gx * a.dx_pred[i] + a.kl2 * a.kdxp[i] : gx * a.dx_pred[i];
        a.sc_x[i] = gx * a.dx_corr[i] + (KL ? a.kl2 * a.kdxc[i] : (a.uc_x ? a.uc_x[i] : 0.f));
        return;
    }
    i -= nx;
    if (i < nt) {
        const float gt = a.g[a.B + a.n2g[i / MI_NUM_TYPES]];
        a.sp_t[i] = KL ? gt * a.dt[i] + a.kl1 * a.kdt[i] : gt * a.dt[i];
        a.sc_t[i] = !KL && a.uc_t ? a.uc_t[i] : 0.f;
    }
}

// a handle's buffer set, allocated on first use; the last entry is allocated last, so its presence marks the set complete
static int alloc_set(mi_batch* b, std::initializer_list<std::pair<float**, size_t>> set) {
    if (*(set.end() - 1)->first) return MI_OK;
    for (const auto& e : set) MI_TRY(dev_alloc(b, e.first, e.second));
    return MI_OK;
}

static int traj_buffers(mi_batch* b) {
    const size_t nl = (size_t)b->B * 9, nx = (size_t)b->N * 3, nt = (size_t)b->N * MI_NUM_TYPES;
    return alloc_set(b, {{&b->tr_dl, nl}, {&b->tr_dt, nt}, {&b->tr_sl, nl}, {&b->tr_sx, nx}, {&b->tr_st, nt}, {&b->tr_dx, nx}});
}

static LikMask lik_mask(const mi_batch* b) { return LikMask{b->lik_kt, b->lik_kx, b->lik_kl}; }

static bool same_counts(const mi_batch* p, const mi_batch* q) {
    return p->B == q->B && p->N == q->N && p->num_atoms_h == q->num_atoms_h;
}

// the work of mi_traj_logprob after its argument checks (the times in t_dev are valid): shared with mi_traj_pg_step, which checks its times on the host
static int traj_logprob_enqueue(mi_net* net, mi_batch* bc, mi_batch* bp, const int* t_dev, const float* coef_dev, const float* time_freqs,
                                const float* atom_types, const float* frac, const float* frac_mid, const float* lattices,
                                const float* next_atom_types, const float* next_frac, const float* next_lattices, float* log_prob,
                                float* pred_corr_l, float* pred_corr_x, float* pred_corr_t, int keep_tape, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const int B = bc->B, N = bc->N;
    if (keep_tape) {
        MI_TRY(traj_buffers(bc));
        MI_TRY(traj_buffers(bp));
    }
    // time embedding of each crystal's t (diffusion.py:161), once for both evaluations
    if (bc->time_map) {   // a strided chain: t_dev holds step indices, the network sees the trained times map[t]
        MI_TRY(time_embedding_mapped(bc, t_dev, 0, time_freqs, B, net->TD, bc->temb, s));
    } else {
        MI_TRY(mi_time_embedding(t_dev, time_freqs, B, net->TD, bc->temb, stream));
    }
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
    if (bp->lik_on) {   // a conditioned chain's likelihood; the entries have checked that bc carries the same mask
        hipLaunchKernelGGL(traj_logprob_masked_kernel, dim3(B), dim3(256), 0, s, a, lik_mask(bp));
    } else {
        hipLaunchKernelGGL(traj_logprob_kernel, dim3(B), dim3(256), 0, s, a);
    }
    MI_KERNEL_CHECK();
    if (train && N > 0) {
        bc->tr_partner = bp;
        bc->tr_epoch = bc->fwd_epoch;
        bc->tr_partner_epoch = bp->fwd_epoch;
    }
    return MI_OK;
}

static bool traj_handles_ok(mi_net* net, mi_batch* bc, mi_batch* bp) {
    return bc->H == net->H && bc->L == net->L && bp->H == net->H && bp->L == net->L;
}

// strided chains: the pair shares one time map (or has none), and a map has the call's T + 1 entries; conditioned chains: the pair shares
// one likelihood mask (or has none)
static int traj_time_map_ok(const mi_batch* bc, const mi_batch* bp, int T) {
    MI_TRY(likelihood_mask_same(bc, bp, "the two batch handles carry different likelihood masks (mi_batch_set_likelihood_mask: both, and the same, or neither)"));
    MI_TRY(time_map_same(bc, bp, "the two batch handles carry different time maps"));
    return time_map_check(bc, T, "the batch handle");
}

// ---- the PPO-clipped policy-gradient micro-step (mi_traj_pg_step) ----------------------------------------------------------------

struct GatherArgs {
    const int* t;                                   // [B] caller's times (the host checked its copy: 2..T)
    const int* n2g;                                 // [N]
    const float *ta, *tx, *txm, *tl;                // the rollout: [T+1][N][A], [T+1][N][3] x 2, [T+1][B][9]
    float *a, *x, *xm, *l, *na, *nx, *nl;           // crystal b's state at t_b and t_b - 1
    int* t_out;                                     // [B] the times every later kernel of the micro-step reads
    int B, N, T;
};

__device__ __forceinline__ int pg_time(const int* t, int b, int T) {
    const int v = t[b];
    return v < 2 ? 2 : (v > T ? T : v);   // (the host checked these values: the clamp only keeps every read of a stray one inside the rollout)
}

// one thread per gathered element of the seven arrays: N*A (types at t, at t-1), N*3 (coordinates at t, mid coordinates at t, coordinates at
// t-1), B*9 (lattice at t, at t-1); plain copies, the bits of the record
__global__ __launch_bounds__(256) void traj_pg_gather_kernel(GatherArgs a) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.B) a.t_out[i] = pg_time(a.t, (int)i, a.T);
    const int64_t nt = (int64_t)a.N * MI_NUM_TYPES, nx = (int64_t)a.N * 3, nl = (int64_t)a.B * 9;
    if (i < 2 * nt) {
        const bool next = i >= nt;
        const int64_t e = next ? i - nt : i;
        const int t = pg_time(a.t, a.n2g[e / MI_NUM_TYPES], a.T) - (next ? 1 : 0);
        (next ? a.na : a.a)[e] = a.ta[(int64_t)t * nt + e];
        return;
    }
    i -= 2 * nt;
    if (i < 3 * nx) {
        const int k = (int)(i / nx);
        const int64_t e = i - k * nx;
        const int t = pg_time(a.t, a.n2g[e / 3], a.T) - (k == 2 ? 1 : 0);
        const float* src = k == 1 ? a.txm : a.tx;
        float* dst = k == 0 ? a.x : (k == 1 ? a.xm : a.nx);
        dst[e] = src[(int64_t)t * nx + e];
        return;
    }
    i -= 3 * nx;
    if (i < 2 * nl) {
        const bool next = i >= nl;
        const int64_t e = next ? i - nl : i;
        const int t = pg_time(a.t, (int)(e / 9), a.T) - (next ? 1 : 0);
        (next ? a.nl : a.l)[e] = a.tl[(int64_t)t * nl + e];
    }
}

struct SurrogateArgs {
    const int* t;          // [B] (checked)
    const float* lp;       // [3][B] new log-probabilities
    const float* lp_old;   // [T+1][B][3] the sampler's record
    const float* adv;      // [B]
    float* g;              // [3][B] seeds
    float* stats;          // [4][B] running sums
    float w0, w1, w2, lo, hi, eps, scale;
    int B;
};

// one thread per crystal: the clipped surrogate, its upstream gradient and the running statistics -- each crystal's sums owned by one thread
__global__ __launch_bounds__(256) void traj_pg_surrogate_kernel(SurrogateArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const float* o = a.lp_old + ((int64_t)a.t[b] * a.B + b) * 3;
    const float lp_new = (a.w0 * a.lp[b] + a.w1 * a.lp[a.B + b]) + a.w2 * a.lp[2 * a.B + b];
    const float lp_old = (a.w0 * o[0] + a.w1 * o[1]) + a.w2 * o[2];
    const float d = lp_new - lp_old;
    const float rho = expf(d);
    const float na = -a.adv[b];
    const float rc = rho < a.lo ? a.lo : (rho > a.hi ? a.hi : rho);   // torch.clamp (NaN passes through)
    const float u = na * rho, c = na * rc;
    const float L = u > c ? u : c;
    const bool unclipped = !(rho < a.lo || rho > a.hi) || u > c;
    const float g = unclipped ? (a.scale * na) * rho : 0.f;
    a.g[b] = a.w0 * g;
    a.g[a.B + b] = a.w1 * g;
    a.g[2 * a.B + b] = a.w2 * g;
    a.stats[b] += L;
    a.stats[a.B + b] += rho;
    a.stats[2 * a.B + b] += 0.5f * (d * d);
    a.stats[3 * a.B + b] += fabsf(rho - 1.0f) > a.eps ? 1.0f : 0.0f;
}

static int pg_buffers(mi_batch* b) {
    const size_t nt = (size_t)b->N * MI_NUM_TYPES, nx = (size_t)b->N * 3, nl = (size_t)b->B * 9, n3 = (size_t)3 * b->B;
    if (!b->pg_t) MI_TRY(dev_alloc(b, &b->pg_t, (size_t)b->B));
    return alloc_set(b, {{&b->pg_a, nt}, {&b->pg_na, nt}, {&b->pg_x, nx}, {&b->pg_xm, nx}, {&b->pg_nx, nx}, {&b->pg_l, nl}, {&b->pg_nl, nl},
                         {&b->pg_lp, n3}, {&b->pg_g, n3}});
}

// the argument checks of a policy-gradient micro-step, all on the host, before anything is enqueued (the kernels index the rollout with the times)
static int pg_check(mi_net* net, mi_batch* bc, mi_batch* bp, const float* coef_dev, int T, const float* time_freqs, const float* traj_atom_types,
                    const float* traj_frac, const float* traj_frac_mid, const float* traj_lattices, const float* traj_lp_old, const int* t_host,
                    const int* t_dev, const float* adv_dev, float clip_range, const float* w_host, const float* grad_theta, const float* stats) {
    MI_CHECK(net && bc && bp, MI_EINVAL, "null handle");
    MI_CHECK(bc != bp, MI_EINVAL, "the corrector and the predictor evaluation need two distinct batch handles");
    MI_CHECK(traj_handles_ok(net, bc, bp), MI_EINVAL, "batch was created for a different network");
    MI_CHECK(same_counts(bc, bp), MI_EINVAL, "the two batch handles hold different atom counts");
    MI_CHECK(coef_dev && time_freqs && traj_atom_types && traj_frac && traj_frac_mid && traj_lattices && traj_lp_old && t_host && t_dev &&
                 adv_dev && w_host && grad_theta && stats, MI_EINVAL, "null argument");
    MI_CHECK(T >= 2, MI_EINVAL, "T = %d: a recorded step needs T >= 2", T);
    MI_TRY(traj_time_map_ok(bc, bp, T));
    MI_CHECK(clip_range >= 0.f, MI_EINVAL, "clip_range = %g: must be >= 0", (double)clip_range);
    MI_CHECK(net->W2T != nullptr, MI_ESTATE, "mi_net_set_params must run before backward");
    for (int i = 0; i < bc->B; ++i)
        MI_CHECK(t_host[i] >= 2 && t_host[i] <= T, MI_EINVAL, "t[%d] = %d: a recorded step has t in 2..T = %d", i, t_host[i], T);
    return MI_OK;
}

// one gather launch: crystal b's state at t_b and t_b - 1 into bc's pg_* buffers, the checked times into pg_t
static int pg_gather(mi_batch* bc, int T, const int* t_dev, const float* ta, const float* tx, const float* txm, const float* tl, hipStream_t s) {
    const int B = bc->B, N = bc->N;
    GatherArgs g;
    g.t = t_dev, g.n2g = bc->node2graph;
    g.ta = ta, g.tx = tx, g.txm = txm, g.tl = tl;
    g.a = bc->pg_a, g.x = bc->pg_x, g.xm = bc->pg_xm, g.l = bc->pg_l, g.na = bc->pg_na, g.nx = bc->pg_nx, g.nl = bc->pg_nl;
    g.t_out = bc->pg_t;
    g.B = B, g.N = N, g.T = T;
    const int64_t ng = 2 * (int64_t)N * MI_NUM_TYPES + 9 * (int64_t)N + 18 * (int64_t)B;
    hipLaunchKernelGGL(traj_pg_gather_kernel, dim3(cdiv(ng, 256)), dim3(256), 0, s, g);
    MI_KERNEL_CHECK();
    return MI_OK;
}

// one surrogate launch: seeds into bc->pg_g, statistics rows 0..3
static int pg_surrogate(mi_batch* bc, const float* lp, const float* traj_lp_old, const float* adv_dev, float clip_range, const float* w_host,
                        float loss_scale, float* stats, hipStream_t s) {
    const int B = bc->B;
    SurrogateArgs u;
    u.t = bc->pg_t, u.lp = lp, u.lp_old = traj_lp_old, u.adv = adv_dev, u.g = bc->pg_g, u.stats = stats;
    u.w0 = w_host[0], u.w1 = w_host[1], u.w2 = w_host[2];
    u.lo = (float)(1.0 - (double)clip_range), u.hi = (float)(1.0 + (double)clip_range), u.eps = clip_range;
    u.scale = loss_scale;
    u.B = B;
    hipLaunchKernelGGL(traj_pg_surrogate_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, u);
    MI_KERNEL_CHECK();
    return MI_OK;
}

// ---- the KL anchor to a frozen prior (mi_traj_pg_kl_step) ---------------------------------------------------------------------------

struct KlArgs {
    const int* t;                                   // [B] (checked)
    const float* coef;                              // [T+1][MI_NCOEF]
    const int* node_off;                            // [B+1]
    const float *pxc_a, *pl_a, *pxp_a, *pt_a;       // the agent: corrector coordinate head; predictor's three heads
    const float *pxc_p, *pl_p, *pxp_p, *pt_p;       // the prior, same
    float *dl, *dt, *dxc, *dxp;                     // d KL_k / d(agent output): [B][9], [N][A], [N][3], [N][3]
    float* kl;                                      // [3][B] (KL_l, KL_t, KL_x)
    float* stats;                                   // [B] row 4 of the statistics: += w . KL
    float w0, w1, w2;
    int B;
};

// one 256-thread block per crystal, the thread-to-element maps and reduction trees of traj_logprob_kernel: no atomics, same bits every call.
// Every difference is taken between the two predictions, never between the two rounded means.
// MASK: as traj_logprob_masked_kernel's -- the predictor's lattice, type and coordinate terms of the known elements leave the sums, their
// derivatives are 0.f; the corrector coordinate term and the divisors stay.  traj_pg_kl_kernel is this body with MASK = false.
template <bool MASK>
__device__ __forceinline__ void traj_pg_kl_body(KlArgs a, LikMask m) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const StepCoef c = load_coef(a.coef, a.t[b]);
    const int n0 = a.node_off[b], n1 = a.node_off[b + 1], n = n1 - n0;
    const float cnt = (float)(n > 0 ? n : 1);

    // coordinates: mu_a - mu_p = -s (p_a - p_p) on the torus, s = step * sqrt(sn); its nearest image mi(d) = d - rint(d); KL = mi^2 / (2 std^2),
    // d KL / d p_a = mi * s / std^2, each coordinate with weight 1 / (3 n)
    const float sc = c.step_corr * c.sqrt_sn, sp = c.step_pred * c.sqrt_sn;
    const float kc = sc / c.std_corr_sq / 3.0f / cnt, kp = sp / c.std_pred_sq / 3.0f / cnt;
    float klc = 0.f, klp = 0.f;
    for (int idx = n0 * 3 + tid; idx < n1 * 3; idx += 256) {
        float d = sc * (a.pxc_a[idx] - a.pxc_p[idx]);
        d = d - rintf(d);
        klc += (d * d) / (2.0f * c.std_corr_sq);
        a.dxc[idx] = d * kc;
        if (MASK && m.known_coords[idx / 3]) {
            a.dxp[idx] = 0.f;
            continue;
        }
        d = sp * (a.pxp_a[idx] - a.pxp_p[idx]);
        d = d - rintf(d);
        klp += (d * d) / (2.0f * c.std_pred_sq);
        a.dxp[idx] = d * kp;
    }
    klc = block_sum_256(klc, red);
    klp = block_sum_256(klp, red);

    // lattice: m_a - m_p = -c0 c1 (pl_a - pl_p); KL = 1/9 sum (c0 c1 d)^2 / (2 sigma^2), d KL / d pl_a = c0 c1 (c0 c1 d) / (9 sigma^2)
    const float cc = c.c0 * c.c1;
    float kll = 0.f;
    if (tid < 9) {
        const int idx = b * 9 + tid;
        if (MASK && m.known_lattice[b]) {
            a.dl[idx] = 0.f;
        } else {
            const float d = cc * (a.pl_a[idx] - a.pl_p[idx]);
            kll = (d * d) / (2.0f * c.sigma_sq);
            a.dl[idx] = d * cc / c.sigma_sq / 9.0f;
        }
    }
    kll = block_sum_256(kll, red);

    // atom-type logits: the same Normal, mean over the 100 logits, then over the atoms; one wave per atom
    const int lane = tid & 63, wave = tid >> 6;
    const float kt = cc / c.sigma_sq / (float)MI_NUM_TYPES / cnt;
    float klt = 0.f;
    for (int i = n0 + wave; i < n1; i += 4) {
        if (MASK && m.known_types[i]) {
            for (int k = lane; k < MI_NUM_TYPES; k += 64) a.dt[(size_t)i * MI_NUM_TYPES + k] = 0.f;
            continue;
        }
        float s = 0.f;
        for (int k = lane; k < MI_NUM_TYPES; k += 64) {
            const size_t idx = (size_t)i * MI_NUM_TYPES + k;
            const float d = cc * (a.pt_a[idx] - a.pt_p[idx]);
            s += (d * d) / (2.0f * c.sigma_sq);
            a.dt[idx] = d * kt;
        }
        s = wave_sum(s);
        klt += s / (float)MI_NUM_TYPES;
    }
    __syncthreads();
    if (lane == 0) red[wave] = klt;
    __syncthreads();
    if (tid == 0) {
        const float l = kll / 9.0f;
        const float t = ((red[0] + red[1]) + (red[2] + red[3])) / cnt;
        const float x = (klc / 3.0f) / cnt + (klp / 3.0f) / cnt;
        a.kl[b] = l;
        a.kl[a.B + b] = t;
        a.kl[2 * a.B + b] = x;
        a.stats[b] += (a.w0 * l + a.w1 * t) + a.w2 * x;
    }
}

__global__ __launch_bounds__(256) void traj_pg_kl_kernel(KlArgs a) {
    traj_pg_kl_body<false>(a, LikMask{nullptr, nullptr, nullptr});
}

__global__ __launch_bounds__(256) void traj_pg_kl_masked_kernel(KlArgs a, LikMask m) {
    traj_pg_kl_body<true>(a, m);
}

static int kl_buffers(mi_batch* bc, mi_batch* pb) {
    const size_t nt = (size_t)bc->N * MI_NUM_TYPES, nx = (size_t)bc->N * 3, nl = (size_t)bc->B * 9;
    MI_TRY(alloc_set(pb, {{&pb->kl_pxc, (size_t)pb->N * 3}}));
    return alloc_set(bc, {{&bc->kl_dt, nt}, {&bc->kl_dxc, nx}, {&bc->kl_dxp, nx}, {&bc->kl_val, (size_t)3 * bc->B}, {&bc->kl_dl, nl}});
}

// one KL launch: per-term KL into `kl`, their weighted sum onto statistics row 4, the local derivatives into bc's kl_d* buffers
static int kl_launch(mi_batch* bc, mi_batch* bp, mi_batch* pb, const float* coef_dev, const float* w_host, float* kl, float* stats, hipStream_t s) {
    KlArgs k;
    k.t = bc->pg_t, k.coef = coef_dev, k.node_off = bc->node_off;
    k.pxc_a = bc->pred_x, k.pl_a = bp->pred_l, k.pxp_a = bp->pred_x, k.pt_a = bp->pred_t;
    k.pxc_p = pb->kl_pxc, k.pl_p = pb->pred_l, k.pxp_p = pb->pred_x, k.pt_p = pb->pred_t;
    k.dl = bc->kl_dl, k.dt = bc->kl_dt, k.dxc = bc->kl_dxc, k.dxp = bc->kl_dxp;
    k.kl = kl;
    k.stats = stats + 4 * (size_t)bc->B;
    k.w0 = w_host[0], k.w1 = w_host[1], k.w2 = w_host[2];
    k.B = bc->B;
    if (bp->lik_on) {
        hipLaunchKernelGGL(traj_pg_kl_masked_kernel, dim3(bc->B), dim3(256), 0, s, k, lik_mask(bp));
    } else {
        hipLaunchKernelGGL(traj_pg_kl_kernel, dim3(bc->B), dim3(256), 0, s, k);
    }
    MI_KERNEL_CHECK();
    return MI_OK;
}

// the seeds of both evaluations of the taped call pending on (bc, bp), then one backward per evaluation.  kl_w NULL: seeds from the upstream
// gradients g and d_corr_* (each may be NULL); else g plus kl_w[k] times the KL derivatives in bc's kl_d* buffers.
static int traj_seed_backward(mi_net* net, mi_batch* bc, mi_batch* bp, const float* g, const float* d_corr_l, const float* d_corr_x,
                              const float* d_corr_t, const float* kl_w, float* grad_theta, hipStream_t s) {
    const int B = bc->B, N = bc->N;
    SeedArgs a;
    a.g = g;
    a.n2g = bc->node2graph;
    a.dl = bp->tr_dl, a.dx_corr = bc->tr_dx, a.dx_pred = bp->tr_dx, a.dt = bp->tr_dt;
    a.uc_l = d_corr_l, a.uc_x = d_corr_x, a.uc_t = d_corr_t;
    a.kdl = bc->kl_dl, a.kdxc = bc->kl_dxc, a.kdxp = bc->kl_dxp, a.kdt = bc->kl_dt;
    a.kl0 = kl_w ? kl_w[0] : 0.f, a.kl1 = kl_w ? kl_w[1] : 0.f, a.kl2 = kl_w ? kl_w[2] : 0.f;
    a.sc_l = bc->tr_sl, a.sc_x = bc->tr_sx, a.sc_t = bc->tr_st;
    a.sp_l = bp->tr_sl, a.sp_x = bp->tr_sx, a.sp_t = bp->tr_st;
    a.B = B, a.N = N;
    const int64_t n = (int64_t)B * 9 + (int64_t)N * (3 + MI_NUM_TYPES);
    if (kl_w) {
        hipLaunchKernelGGL(traj_seed_kernel<true>, dim3(cdiv(n, 256)), dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL(traj_seed_kernel<false>, dim3(cdiv(n, 256)), dim3(256), 0, s, a);
    }
    MI_KERNEL_CHECK();
    MI_TRY(net_backward(net, bp, bp->tr_sl, bp->tr_sx, bp->tr_st, grad_theta, s));
    return net_backward(net, bc, bc->tr_sl, bc->tr_sx, bc->tr_st, grad_theta, s);
}

// The policy-gradient micro-step after its argument checks (pg_check; with a prior, the entry's own), everything enqueued, no host
// synchronisation.  prior / pb NULL: the clipped surrogate alone (mi_traj_pg_step); else with the KL anchor (mi_traj_pg_kl_step).
//   1. the buffers, on first use
//   2. the gather: crystal b's recorded state at t_b and t_b - 1
//   3. (prior) its time embedding and two inference evaluations of the gathered state -- on aux_stream if there is one, forked after the gather
//   4. the agent's two taped evaluations and the log-probabilities
//   5. (prior) the join, then the KL and its local derivatives
//   6. the surrogate: upstream gradients and statistics
//   7. the seeds of both evaluations (surrogate, + KL with a prior)
//   8. one backward per evaluation into grad_theta
// The seeds go straight to traj_seed_backward: mi_traj_logprob_backward's check of the tape state could not fire here, step 4 has just set it.
static int pg_enqueue(mi_net* net, mi_batch* bc, mi_batch* bp, mi_net* prior, mi_batch* pb, const float* coef_dev, int T, const float* time_freqs,
                      const float* traj_atom_types, const float* traj_frac, const float* traj_frac_mid, const float* traj_lattices,
                      const float* traj_lp_old, const int* t_dev, const float* adv_dev, float clip_range, const float* w_host, float loss_scale,
                      float kl_coef, float* log_prob, float* kl_out, float* grad_theta, float* stats, void* stream, void* aux_stream) {
    if (bc->B == 0 || bc->N == 0) return MI_OK;
    MI_TRY(pg_buffers(bc));
    if (prior) MI_TRY(kl_buffers(bc, pb));
    hipStream_t s = (hipStream_t)stream;
    const bool aux = prior && aux_stream && aux_stream != stream;
    MI_TRY(pg_gather(bc, T, t_dev, traj_atom_types, traj_frac, traj_frac_mid, traj_lattices, s));
    if (prior) {
        hipStream_t sp = aux ? (hipStream_t)aux_stream : s;
        if (pb->time_map) {   // (the entry has checked that it is the agent handles' map)
            MI_TRY(time_embedding_mapped(pb, bc->pg_t, 0, time_freqs, bc->B, prior->TD, pb->temb, s));
        } else {
            MI_TRY(mi_time_embedding(bc->pg_t, time_freqs, bc->B, prior->TD, pb->temb, stream));
        }
        if (aux) {
            if (!pb->ev_fork) {
                MI_HIP(hipEventCreateWithFlags(&pb->ev_fork, hipEventDisableTiming));
                MI_HIP(hipEventCreateWithFlags(&pb->ev_join, hipEventDisableTiming));
            }
            MI_HIP(hipEventRecord(pb->ev_fork, s));
            MI_HIP(hipStreamWaitEvent(sp, pb->ev_fork, 0));
        }
        // (the corrector evaluation's coordinate head alone is read: its lattice / type heads land in pred_l / pred_t, which the predictor overwrites)
        MI_TRY(net_forward(prior, pb, pb->temb, bc->pg_a, bc->pg_x, bc->pg_l, pb->pred_l, pb->kl_pxc, pb->pred_t, sp, false, false, true));
        MI_TRY(net_forward(prior, pb, pb->temb, bc->pg_a, bc->pg_xm, bc->pg_l, pb->pred_l, pb->pred_x, pb->pred_t, sp, false));
        if (aux) MI_HIP(hipEventRecord(pb->ev_join, sp));
    }
    float* lp = log_prob ? log_prob : bc->pg_lp;
    MI_TRY(traj_logprob_enqueue(net, bc, bp, bc->pg_t, coef_dev, time_freqs, bc->pg_a, bc->pg_x, bc->pg_xm, bc->pg_l, bc->pg_na, bc->pg_nx,
                                bc->pg_nl, lp, nullptr, nullptr, nullptr, 1, stream));
    if (aux) MI_HIP(hipStreamWaitEvent(s, pb->ev_join, 0));
    if (prior) MI_TRY(kl_launch(bc, bp, pb, coef_dev, w_host, kl_out ? kl_out : bc->kl_val, stats, s));
    MI_TRY(pg_surrogate(bc, lp, traj_lp_old, adv_dev, clip_range, w_host, loss_scale, stats, s));
    const float kc = kl_coef * loss_scale;
    const float kl_w[3] = {kc * w_host[0], kc * w_host[1], kc * w_host[2]};
    return traj_seed_backward(net, bc, bp, bc->pg_g, nullptr, nullptr, nullptr, prior ? kl_w : nullptr, grad_theta, s);
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_traj_logprob(mi_net* net, mi_batch* bc, mi_batch* bp, const int* t_dev, const float* coef_dev, int T, const float* time_freqs,
                    const float* atom_types, const float* frac, const float* frac_mid, const float* lattices, const float* next_atom_types,
                    const float* next_frac, const float* next_lattices, float* log_prob, float* pred_corr_l, float* pred_corr_x,
                    float* pred_corr_t, int keep_tape, void* stream) {
    MI_NO_LATENT(net, "mi_traj_logprob");
    MI_NO_POOLED(bc, "mi_traj_logprob");
    MI_NO_POOLED(bp, "mi_traj_logprob");
    MI_CHECK(net && bc && bp, MI_EINVAL, "null handle");
    MI_CHECK(bc != bp, MI_EINVAL, "the corrector and the predictor evaluation need two distinct batch handles");
    MI_CHECK(traj_handles_ok(net, bc, bp), MI_EINVAL, "batch was created for a different network");
    MI_CHECK(same_counts(bc, bp), MI_EINVAL, "the two batch handles hold different atom counts");
    MI_CHECK(t_dev && coef_dev && time_freqs && atom_types && frac && frac_mid && lattices && next_atom_types && next_frac && next_lattices &&
                 log_prob, MI_EINVAL, "null argument");
    MI_CHECK(T >= 2, MI_EINVAL, "T = %d: a recorded step needs T >= 2", T);
    MI_TRY(traj_time_map_ok(bc, bp, T));
    hipStream_t s = (hipStream_t)stream;
    const int B = bc->B;
    bc->tr_partner = nullptr;   // whatever was pending on this pair is about to be overwritten
    if (B == 0) return MI_OK;
    std::vector<int> th(B);
    MI_HIP(hipMemcpyAsync(th.data(), t_dev, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < B; ++i)
        MI_CHECK(th[i] >= 2 && th[i] <= T, MI_EINVAL, "timesteps[%d] = %d: a recorded step has t in 2..T = %d", i, th[i], T);
    return traj_logprob_enqueue(net, bc, bp, t_dev, coef_dev, time_freqs, atom_types, frac, frac_mid, lattices, next_atom_types, next_frac,
                                next_lattices, log_prob, pred_corr_l, pred_corr_x, pred_corr_t, keep_tape, stream);
}

int mi_traj_logprob_backward(mi_net* net, mi_batch* bc, mi_batch* bp, const float* g_logp, const float* d_corr_l, const float* d_corr_x,
                             const float* d_corr_t, float* grad_theta, void* stream) {
    MI_NO_POOLED(bc, "mi_traj_logprob_backward");
    MI_NO_POOLED(bp, "mi_traj_logprob_backward");
    MI_CHECK(net && bc && bp && g_logp && grad_theta, MI_EINVAL, "null argument");
    MI_CHECK(net->W2T != nullptr, MI_ESTATE, "mi_net_set_params must run before backward");
    if (bc->B == 0 || bc->N == 0) return MI_OK;
    MI_CHECK(bc->tr_partner == bp && bc->tr_epoch == bc->fwd_epoch && bp->fwd_epoch == bc->tr_partner_epoch && bc->tape.valid && bp->tape.valid,
             MI_ESTATE, "mi_traj_logprob_backward: no taped mi_traj_logprob pending on these handles (not taped, or a later evaluation overwrote it)");
    return traj_seed_backward(net, bc, bp, g_logp, d_corr_l, d_corr_x, d_corr_t, nullptr, grad_theta, (hipStream_t)stream);
}

int mi_traj_read_derivatives(const mi_batch* b, float* dl, float* dx, float* dt, void* stream) {
    MI_NO_POOLED(b, "mi_traj_read_derivatives");
    MI_CHECK(b, MI_EINVAL, "null handle");
    MI_CHECK(b->tr_dl && b->tr_dx && b->tr_dt, MI_ESTATE, "mi_traj_read_derivatives: no taped call has used this handle");
    hipStream_t s = (hipStream_t)stream;
    if (dl && b->B) MI_HIP(hipMemcpyAsync(dl, b->tr_dl, (size_t)b->B * 9 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (dx && b->N) MI_HIP(hipMemcpyAsync(dx, b->tr_dx, (size_t)b->N * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (dt && b->N) MI_HIP(hipMemcpyAsync(dt, b->tr_dt, (size_t)b->N * MI_NUM_TYPES * sizeof(float), hipMemcpyDeviceToDevice, s));
    return MI_OK;
}

int mi_traj_pg_step(mi_net* net, mi_batch* bc, mi_batch* bp, const float* coef_dev, int T, const float* time_freqs,
                    const float* traj_atom_types, const float* traj_frac, const float* traj_frac_mid, const float* traj_lattices,
                    const float* traj_lp_old, const int* t_host, const int* t_dev, const float* adv_dev, float clip_range,
                    const float* w_host, float loss_scale, float* log_prob, float* grad_theta, float* stats, void* stream) {
    MI_NO_LATENT(net, "mi_traj_pg_step");
    MI_NO_POOLED(bc, "mi_traj_pg_step");
    MI_NO_POOLED(bp, "mi_traj_pg_step");
    MI_TRY(pg_check(net, bc, bp, coef_dev, T, time_freqs, traj_atom_types, traj_frac, traj_frac_mid, traj_lattices, traj_lp_old, t_host, t_dev,
                    adv_dev, clip_range, w_host, grad_theta, stats));
    return pg_enqueue(net, bc, bp, nullptr, nullptr, coef_dev, T, time_freqs, traj_atom_types, traj_frac, traj_frac_mid, traj_lattices, traj_lp_old,
                      t_dev, adv_dev, clip_range, w_host, loss_scale, 0.f, log_prob, nullptr, grad_theta, stats, stream, nullptr);
}

int mi_traj_pg_kl_step(mi_net* net, mi_batch* bc, mi_batch* bp, mi_net* prior, mi_batch* pb, const float* coef_dev, int T,
                       const float* time_freqs, const float* traj_atom_types, const float* traj_frac, const float* traj_frac_mid,
                       const float* traj_lattices, const float* traj_lp_old, const int* t_host, const int* t_dev, const float* adv_dev,
                       float clip_range, const float* w_host, float loss_scale, float kl_coef, float* log_prob, float* kl_out,
                       float* grad_theta, float* stats, void* stream, void* aux_stream) {
    MI_NO_LATENT(net, "mi_traj_pg_kl_step");
    MI_NO_LATENT(prior, "mi_traj_pg_kl_step");
    MI_NO_POOLED(bc, "mi_traj_pg_kl_step");
    MI_NO_POOLED(bp, "mi_traj_pg_kl_step");
    MI_NO_POOLED(pb, "mi_traj_pg_kl_step");
    MI_TRY(pg_check(net, bc, bp, coef_dev, T, time_freqs, traj_atom_types, traj_frac, traj_frac_mid, traj_lattices, traj_lp_old, t_host, t_dev,
                    adv_dev, clip_range, w_host, grad_theta, stats));
    MI_CHECK(prior && pb, MI_EINVAL, "null prior handle");
    MI_CHECK(pb != bc && pb != bp, MI_EINVAL, "the prior needs a batch handle of its own");
    MI_CHECK(pb->H == prior->H && pb->L == prior->L, MI_EINVAL, "prior batch was created for a different network");
    MI_CHECK(same_counts(bc, pb), MI_EINVAL, "the prior's batch handle holds different atom counts");
    MI_TRY(time_map_same(bc, pb, "the prior's batch handle carries another time map than the agent's (a strided chain: both, and the same)"));
    MI_TRY(likelihood_mask_same(bc, pb, "the prior's batch handle carries another likelihood mask than the agent's (a conditioned rollout: all three handles, and the same)"));
    MI_CHECK(prior->TD == net->TD, MI_EINVAL, "the prior's time embedding has %d dimensions, the agent's %d (one frequency table serves both)", prior->TD, net->TD);
    MI_CHECK(kl_coef >= 0.f, MI_EINVAL, "kl_coef = %g: must be >= 0", (double)kl_coef);
    MI_CHECK(prior->theta != nullptr, MI_ESTATE, "mi_net_set_params must run on the prior before it is evaluated");
    return pg_enqueue(net, bc, bp, prior, pb, coef_dev, T, time_freqs, traj_atom_types, traj_frac, traj_frac_mid, traj_lattices, traj_lp_old,
                      t_dev, adv_dev, clip_range, w_host, loss_scale, kl_coef, log_prob, kl_out, grad_theta, stats, stream, aux_stream);
}

}  // extern "C"
