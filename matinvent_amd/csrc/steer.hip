// Predictor-steered sampling (include/matinvent_hip_steer.h): the noise-aware predictor's two entries -- input stages of
// scalar_head.hip's scalar_run, whose head, loss, statistics and backward they share -- and the particle resampling.  Launches of this
// unit, no atomics:
//   steer_time_kernel     one thread per crystal: the time clamped to 0..T and the crystal's schedule row;
//   steer_temb_kernel     one block per crystal: the time-embedding row of a state's evaluation;
//   steer_plan_kernel     one 64-lane block per particle group: scores and log-weights in parallel, then steer_plan.h on lane 0;
//   steer_gather_kernel   one block per crystal: the ancestor's rows; one more block: the statistics over the groups in a fixed order.
// The plan mirrors separately rounded fp32 operations (tests/steer_ref.py): no contraction into FMAs in this unit.
#pragma clang fp contract(off)

#include <cmath>

#include "../../include/matinvent_hip_steer.h"
#include "net.h"
#include "steer_plan.h"

namespace mi {

static_assert(STEER_MAX_K == MI_STEER_MAX_PARTICLES && DRAW_STEER == MI_STEER_DRAW, "steer_plan.h / common.h and the public header disagree");
static_assert(STEER_MODE_MAX == MI_STEER_MODE_MAX && STEER_MODE_MIN == MI_STEER_MODE_MIN && STEER_MODE_TARGET == MI_STEER_MODE_TARGET, "modes");

// times[c] = clamp(t[c], 0, T) (the host checked these values: the clamp only keeps the read of a stray one inside the table) and
// sched[c] = table[times[c]]; pretrain_time_kernel with the clean row 0 admitted
__global__ __launch_bounds__(256) void steer_time_kernel(const int* __restrict__ t, const float* __restrict__ table, int* __restrict__ times,
                                                         float* __restrict__ sched, int B, int T) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= B) return;
    const int v = t[c], tc = v < 0 ? 0 : (v > T ? T : v);
    times[c] = tc;
#pragma unroll
    for (int k = 0; k < 4; ++k) sched[c * 4 + k] = table[tc * 4 + k];
}

// scalar_inputs_kernel's time-embedding row, alone: the state's arrays are read where they are
__global__ __launch_bounds__(256) void steer_temb_kernel(const float* __restrict__ freqs, const int* __restrict__ times, int t_all, int TD,
                                                         float* __restrict__ temb) {
    const int b = blockIdx.x, half = TD / 2;
    const float t = (float)(times ? times[b] : t_all);
    for (int k = threadIdx.x; k < TD; k += 256) {
        const float arg = t * freqs[k < half ? k : k - half];
        temb[(size_t)b * TD + k] = k < half ? sinf(arg) : cosf(arg);
    }
}

struct SteerPlanArgs {
    const float* out;   // [B][P]
    float *u_prev, *logw;   // [B]
    int* ancestors;     // [B]
    float* parts;       // [G][2] = (flags, ESS)
    int K, P, p, mode;
    float target, lambda, ess_frac;
    uint64_t seed;
    uint32_t level;
    int64_t graph_offset;
};
// One wave per group.  Lanes own the particles k = lane, lane + 64, ...: score and log-weight into LDS; lane 0 then runs the sequential
// plan (at most 256 particles: a few microseconds) and the lanes write the group's results back.
__global__ __launch_bounds__(64) void steer_plan_kernel(SteerPlanArgs a) {
    __shared__ float u[STEER_MAX_K], lw[STEER_MAX_K], w[STEER_MAX_K], up[STEER_MAX_K], lo[STEER_MAX_K];
    __shared__ int anc[STEER_MAX_K];
    __shared__ int flags_s;
    const int g = blockIdx.x, lane = threadIdx.x, K = a.K;
    const int c0 = g * K;
    for (int k = lane; k < K; k += 64) {
        const float o = a.out[(size_t)(c0 + k) * a.P + a.p];
        const float uk = steer_score(o, a.mode, a.target);
        const float pv = a.u_prev[c0 + k], lg = a.logw[c0 + k];
        u[k] = uk;
        up[k] = pv;
        lo[k] = lg;
        lw[k] = steer_logweight(lg, a.lambda, uk, pv);
    }
    __syncthreads();
    if (lane == 0) {
        const float U = philox_uniform1(a.seed, a.level, DRAW_STEER, (uint64_t)(a.graph_offset + c0));
        float ess;
        const int fl = steer_plan_group(K, u, lw, a.ess_frac, U, w, anc, up, lo, &ess);
        flags_s = fl;
        a.parts[g * 2] = (float)fl;
        a.parts[g * 2 + 1] = ess;
    }
    __syncthreads();
    const bool keep = (flags_s & STEER_NO_FINITE) != 0;   // (uniform over the block) u_prev and logw stay what they were
    for (int k = lane; k < K; k += 64) {
        a.ancestors[c0 + k] = c0 + anc[k];
        if (!keep) {
            a.u_prev[c0 + k] = up[k];
            a.logw[c0 + k] = lo[k];
        }
    }
}

struct SteerGatherArgs {
    const int *ancestors, *node_off;
    const float *src_types, *src_frac, *src_lat;
    float *dst_types, *dst_frac, *dst_lat;
    const float* parts;
    float* stats;   // or NULL
    int B, K, G, vec;
};
// Blocks 0 .. B - 1: crystal c takes the rows of crystal ancestors[c] (clamped into c's group: a stray index never leaves it; the host
// checked that the group's members have one atom count).  Type rows are 400 bytes: a multiple of 16, so with 16-byte aligned arrays
// (`vec`, decided on the host) they move as f32x4.  Block B: the statistics, thread i over the groups i, i + 256, ... in that order, then
// the fixed tree.
__global__ __launch_bounds__(256) void steer_gather_kernel(SteerGatherArgs a) {
    const int c = blockIdx.x, tid = threadIdx.x;
    if (c == a.B) {
        __shared__ float red[3][4];
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int g = tid; g < a.G; g += 256) {
            const int fl = (int)a.parts[g * 2];
            s0 += (fl & STEER_RESAMPLED) ? 1.f : 0.f;
            s1 += a.parts[g * 2 + 1];
            s2 += (fl & STEER_NO_FINITE) ? 1.f : 0.f;
        }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        if ((tid & 63) == 0) {
            red[0][tid >> 6] = s0;
            red[1][tid >> 6] = s1;
            red[2][tid >> 6] = s2;
        }
        __syncthreads();
        if (tid < 3) a.stats[tid] += (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
        return;
    }
    const int g0 = (c / a.K) * a.K;
    int src = a.ancestors[c];
    src = src < g0 ? g0 : (src > g0 + a.K - 1 ? g0 + a.K - 1 : src);
    const int d0 = a.node_off[c], n = a.node_off[c + 1] - d0, s0 = a.node_off[src];
    if (tid < 9) a.dst_lat[c * 9 + tid] = a.src_lat[src * 9 + tid];
    for (int i = tid; i < n * 3; i += 256) a.dst_frac[(size_t)d0 * 3 + i] = a.src_frac[(size_t)s0 * 3 + i];
    const size_t dt = (size_t)d0 * MI_NUM_TYPES, st = (size_t)s0 * MI_NUM_TYPES;
    if (a.vec) {
        const f32x4* sp = reinterpret_cast<const f32x4*>(a.src_types + st);
        f32x4* dp = reinterpret_cast<f32x4*>(a.dst_types + dt);
        for (int i = tid; i < n * (MI_NUM_TYPES / 4); i += 256) dp[i] = sp[i];
    } else {
        for (int i = tid; i < n * MI_NUM_TYPES; i += 256) a.dst_types[dt + i] = a.src_types[st + i];
    }
}

// ---- the predictor's input stages ----------------------------------------------------------------------------------------------------

struct NoisedCtx {
    const float *lengths, *angles, *frac0;
    const int* atom_types;
    const float* time_freqs;
    const int* t_dev;
    const float* table;
    int T;
    uint64_t seed;
    uint32_t noise_step;
    const float *rand_l, *rand_x, *rand_t;
    void* stream;
};
// mi_pretrain_micro_step's steps 1-2 with the times 0..T: the time gather, the time embedding, the forward noising into the stage's arrays
static int noised_stage(mi_net* net, mi_batch* b, ScalarStageIO* io, void* ctx, hipStream_t s) {
    const NoisedCtx& c = *static_cast<const NoisedCtx*>(ctx);
    const int B = b->B, N = b->N;
    if (!b->st_sched) MI_TRY(dev_alloc(b, &b->st_sched, (size_t)B * 4));
    const size_t nx = (size_t)N * 3, nl = (size_t)B * 9, nt = (size_t)N * MI_NUM_TYPES;
    if (!io->train && !b->st_noise) MI_TRY(dev_alloc(b, &b->st_noise, nx + nl + nt));
    Tape& tp = b->tape;
    float* const tar_x = io->train ? tp.tar_x : b->st_noise;
    float* const rnd_l = io->train ? tp.rnd_l : b->st_noise + nx;
    float* const rnd_t = io->train ? tp.rnd_t : b->st_noise + nx + nl;
    hipLaunchKernelGGL(steer_time_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, c.t_dev, c.table, b->times, b->st_sched, B, c.T);
    MI_KERNEL_CHECK();
    MI_TRY(mi_time_embedding(b->times, c.time_freqs, B, net->TD, b->temb, s));
    return mi_add_noise_per_crystal(b, c.lengths, c.angles, c.frac0, c.atom_types, b->st_sched, c.seed, c.noise_step, c.rand_l, c.rand_x, c.rand_t,
                                    io->w_lat, io->w_frac, io->w_types, tar_x, rnd_l, rnd_t, c.stream);
}

int scalar_state_stage(mi_net* net, mi_batch* b, ScalarStageIO* io, void* ctx, hipStream_t s) {   // (net.h: mi_scalar_input_grad's stage too)
    const ScalarStateCtx& c = *static_cast<const ScalarStateCtx*>(ctx);
    hipLaunchKernelGGL(steer_temb_kernel, dim3(b->B), dim3(256), 0, s, c.time_freqs, c.times, c.t_all, net->TD, b->temb);
    MI_KERNEL_CHECK();
    io->in_lat = c.lattices;
    io->in_frac = c.frac;
    io->in_types = c.atom_types;
    return MI_OK;
}

static bool overlap(const float* p, const float* q, size_t n) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q, bytes = n * sizeof(float);
    return a < b + bytes && b < a + bytes;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_scalar_micro_step_noised(mi_net* net, mi_batch* b, const float* lengths, const float* angles, const float* frac0, const int* atom_types,
                                const float* time_freqs, const int* t_host, const int* t_dev, const float* sched_table_dev, int T, uint64_t seed,
                                uint32_t noise_step, const float* rand_l, const float* rand_x, const float* rand_t, const float* W, const float* bias,
                                int P, const float* yhat, const int* have, const int* have_host, const int* count_global,
                                const int* count_global_host, int accum_steps, int loss_kind, float* grad_theta, float* grad_W, float* grad_bias,
                                float* stats, float* out, void* stream) {
    const char* what = "mi_scalar_micro_step_noised";
    MI_NO_LATENT(net, "mi_scalar_micro_step_noised");
    MI_CHECK(T >= 1, MI_EINVAL, "%s: T = %d must be >= 1", what, T);
    if (b && b->B > 0 && b->N > 0) {
        MI_CHECK(lengths && angles && frac0 && atom_types && t_host && t_dev && sched_table_dev, MI_EINVAL, "%s: null argument", what);
        for (int c = 0; c < b->B; ++c)
            MI_CHECK(t_host[c] >= 0 && t_host[c] <= T, MI_EINVAL, "%s: t[%d] = %d: a time lies in 0..T = %d", what, c, t_host[c], T);
    }
    NoisedCtx ctx{lengths, angles, frac0, atom_types, time_freqs, t_dev, sched_table_dev, T, seed, noise_step, rand_l, rand_x, rand_t, stream};
    return scalar_run(what, net, b, lengths, angles, frac0, atom_types, time_freqs, nullptr, 0, W, bias, P, yhat, have, have_host, count_global,
                      count_global_host, accum_steps, loss_kind, grad_theta, grad_W, grad_bias, stats, out, stream, noised_stage, &ctx, false);
}

int mi_scalar_forward_state(mi_net* net, mi_batch* b, const float* atom_types, const float* frac, const float* lattices, const float* time_freqs,
                            const int* times, int t_all, const float* W, const float* bias, int P, float* out, void* stream) {
    const char* what = "mi_scalar_forward_state";
    MI_NO_LATENT(net, "mi_scalar_forward_state");
    MI_CHECK(out, MI_EINVAL, "%s: null argument", what);
    MI_CHECK(!b || b->B == 0 || b->N == 0 || (atom_types && frac && lattices), MI_EINVAL, "%s: null argument", what);
    ScalarStateCtx ctx{atom_types, frac, lattices, time_freqs, times, t_all};
    return scalar_run(what, net, b, nullptr, nullptr, nullptr, nullptr, time_freqs, times, t_all, W, bias, P, nullptr, nullptr, nullptr, nullptr,
                      nullptr, 1, MI_SCALAR_LOSS_MSE, nullptr, nullptr, nullptr, nullptr, out, stream, scalar_state_stage, &ctx, true);
}

int mi_steer_resample(mi_batch* b, int K, const float* out, int P, int p, int mode, float target_hat, float lambda, float ess_frac, uint64_t seed,
                      uint32_t level, float* u_prev, float* logw, const float* src_types, const float* src_frac, const float* src_lat,
                      float* dst_types, float* dst_frac, float* dst_lat, int* ancestors, float* stats, void* stream) {
    const char* what = "mi_steer_resample";
    MI_CHECK(b, MI_EINVAL, "null handle");
    MI_POOL_STREAM(b, stream, "mi_steer_resample");
    MI_CHECK(K >= 1 && K <= MI_STEER_MAX_PARTICLES, MI_EINVAL, "%s: K = %d particles per group: 1..%d", what, K, MI_STEER_MAX_PARTICLES);
    const int B = b->B, N = b->N;
    MI_CHECK(B % K == 0, MI_EINVAL, "%s: the handle's %d crystals are not groups of K = %d replicas (B %% K != 0)", what, B, K);
    for (int c = 0; c < B; ++c)
        MI_CHECK(b->num_atoms_h[(size_t)c] == b->num_atoms_h[(size_t)(c / K) * K], MI_EINVAL,
                 "%s: group %d: crystal %d has %d atoms, the group's first has %d (the K replicas of a group share one atom count)", what, c / K, c,
                 b->num_atoms_h[(size_t)c], b->num_atoms_h[(size_t)(c / K) * K]);
    MI_CHECK(P >= 1 && p >= 0 && p < P, MI_EINVAL, "%s: property p = %d of P = %d", what, p, P);
    MI_CHECK(mode == MI_STEER_MODE_MAX || mode == MI_STEER_MODE_MIN || mode == MI_STEER_MODE_TARGET, MI_EINVAL, "%s: unknown mode %d", what, mode);
    MI_CHECK(std::isfinite(lambda), MI_EINVAL, "%s: lambda is not finite", what);
    MI_CHECK(std::isfinite(ess_frac), MI_EINVAL, "%s: ess_frac is not finite", what);
    MI_CHECK(mode != MI_STEER_MODE_TARGET || std::isfinite(target_hat), MI_EINVAL, "%s: target_hat is not finite", what);
    if (B == 0 || N == 0) return MI_OK;
    MI_CHECK(out && u_prev && logw && src_types && src_frac && src_lat && dst_types && dst_frac && dst_lat && ancestors, MI_EINVAL, "%s: null argument",
             what);
    MI_CHECK(!overlap(src_types, dst_types, (size_t)N * MI_NUM_TYPES) && !overlap(src_frac, dst_frac, (size_t)N * 3) &&
                 !overlap(src_lat, dst_lat, (size_t)B * 9),
             MI_EINVAL, "%s: dst aliases src (the gather reads ancestors' rows while it writes: two state buffers)", what);
    if (!b->st_parts) MI_TRY(dev_alloc(b, &b->st_parts, (size_t)B * 2));
    TraceRange range(what);
    hipStream_t s = (hipStream_t)stream;
    const int G = B / K;
    SteerPlanArgs pa{out, u_prev, logw, ancestors, b->st_parts, K, P, p, mode, target_hat, lambda, ess_frac, seed, level, b->graph_offset};
    hipLaunchKernelGGL(steer_plan_kernel, dim3(G), dim3(64), 0, s, pa);
    MI_KERNEL_CHECK();
    const int vec = (((uintptr_t)src_types | (uintptr_t)dst_types) & 15) == 0 ? 1 : 0;
    SteerGatherArgs ga{ancestors, b->node_off, src_types, src_frac, src_lat, dst_types, dst_frac, dst_lat, b->st_parts, stats, B, K, G, vec};
    hipLaunchKernelGGL(steer_gather_kernel, dim3(B + (stats ? 1 : 0)), dim3(256), 0, s, ga);
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // extern "C"
