// The property predictor (include/matinvent_hip_scalar.h): the CSPNet trunk with a scalar head -- the reference's
// CSPNet(pred_scalar=True), cspnet.py:145-147, 281-284 -- as an inference forward and as one training micro-step.  The trunk is net_forward
// (trunk_only: it ends behind the final LayerNorm) and net_backward (dgf_seed: it starts from d gf alone).  Launches of this unit, no atomics:
//   scalar_inputs_kernel    one block per crystal: the clean network inputs and the crystal's time-embedding row;
//   scalar_head_kernel      one block per crystal: the graph mean, the head, and (with targets) the seeds and the crystal's loss terms;
//   scalar_stats_kernel     one block: the sums over the crystals in a fixed order, the 1 + 3 P statistics;
//   scalar_dgf_kernel       one thread per (crystal, column): dgf = d_out W;
//   scalar_wgrad_kernel     one thread per element of W, and one per bias: the sums over the crystals as a fixed four-way tree;
//   scalar_seed_hf_kernel   one thread per (atom, column): d hf[i] = dgf[g(i)] / n_g (net_backward's seed).
// The head and the loss mirror separately rounded fp32 tensor ops: no contraction into FMAs in the functions marked below.  (The clean
// inputs are built under the unit's default, as add_noise_kernel's are: lattice_matrix and pymod1 of common.h.)

#include "../../include/matinvent_hip_scalar.h"
#include "net.h"

namespace mi {

constexpr int SCALAR_MAX_H = 512;   // (the widest net mi_net_create accepts: scalar_head_kernel keeps a crystal's pooled row in static LDS)

struct ScalarInputArgs {
    const float *lengths, *angles, *frac0;
    const int* atom_types;   // [N] 1..100
    const int* node_off;
    const float* freqs;      // [TD / 2]
    const int* times;        // [B] or NULL: t_all
    int t_all, TD;
    float *in_lat, *in_frac, *in_types, *temb;
};
// add_noise_kernel at (c0, c1, sigma) = (1, 0, 0) without its draws, and time_embedding_kernel's row of the crystal
__global__ __launch_bounds__(256) void scalar_inputs_kernel(ScalarInputArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ float Lm[9];
    if (tid == 0) lattice_matrix(a.lengths + b * 3, a.angles + b * 3, Lm);
    __syncthreads();
    if (tid < 9) a.in_lat[b * 9 + tid] = Lm[tid];
    const int n0 = a.node_off[b], n1 = a.node_off[b + 1];
    for (int idx = n0 * 3 + tid; idx < n1 * 3; idx += 256) a.in_frac[idx] = pymod1(a.frac0[idx]);
    for (int64_t idx = (int64_t)n0 * MI_NUM_TYPES + tid; idx < (int64_t)n1 * MI_NUM_TYPES; idx += 256) {
        const int i = (int)(idx / MI_NUM_TYPES), k = (int)(idx % MI_NUM_TYPES);
        a.in_types[idx] = (a.atom_types[i] - 1 == k) ? 1.f : 0.f;
    }
    const int half = a.TD / 2;
    const float t = (float)(a.times ? a.times[b] : a.t_all);
    for (int k = tid; k < a.TD; k += 256) {
        const float arg = t * a.freqs[k < half ? k : k - half];
        a.temb[(size_t)b * a.TD + k] = k < half ? sinf(arg) : cosf(arg);
    }
}

struct ScalarHeadArgs {
    const float* hf;          // [N][H]
    const int* node_off;
    const float *W, *bias;    // [P][H], [P]
    const float* yhat;        // [B][P] or NULL: no loss
    const int *have, *count_global;   // [B][P], [P]
    float *gf, *out;          // [B][H]; [B][P] or NULL
    float *dout, *parts;      // [B][P], [B][P][3] (written when yhat)
    int H, P, loss_kind, accum_steps;
};
#pragma clang fp contract(off)
// One block per crystal.  gf[f] = (sum over the first half of the atoms + sum over the second half) / n, each half in atom order -- the
// order of lattice_head_kernel's pooling (cspnet.hip); wave w owns the properties w, w + 4, ...: lane l adds W[p][f] gf[f] over
// f = l, l + 64, ... in that order, the 64 lanes through the xor butterfly.
__global__ __launch_bounds__(256) void scalar_head_kernel(ScalarHeadArgs a) {
    __shared__ float gf[SCALAR_MAX_H];
    const int b = blockIdx.x, tid = threadIdx.x, H = a.H, P = a.P;
    const int n0 = a.node_off[b], n1 = a.node_off[b + 1];
    const int mid = n0 + (n1 - n0 + 1) / 2;
    const float cnt = (float)(n1 - n0), d = cnt < 1.f ? 1.f : cnt;
    for (int f = tid; f < H; f += 256) {
        float s0 = 0.f, s1 = 0.f;
        for (int i = n0; i < mid; ++i) s0 += a.hf[(size_t)i * H + f];
        for (int i = mid; i < n1; ++i) s1 += a.hf[(size_t)i * H + f];
        const float v = (s0 + s1) / d;
        gf[f] = v;
        a.gf[(size_t)b * H + f] = v;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int p = wave; p < P; p += 4) {   // (uniform over the wave)
        const float* w = a.W + (size_t)p * H;
        float s = 0.f;
        for (int f = lane; f < H; f += 64) s += w[f] * gf[f];
        s = wave_sum(s);
        if (lane != 0) continue;
        const float o = a.bias[p] + s;
        const size_t k = (size_t)b * P + p;
        if (a.out) a.out[k] = o;
        if (!a.yhat) continue;
        float seed = 0.f, e2 = 0.f, ea = 0.f, pres = 0.f;
        if (a.have[k] != 0) {   // (a missing target's yhat is never read: whatever it holds, NaN included, reaches nothing)
            const float e = o - a.yhat[k];
            const float den = (float)((double)P * (double)a.count_global[p] * (double)a.accum_steps);
            e2 = e * e;
            ea = fabsf(e);
            pres = 1.f;
            seed = a.loss_kind == MI_SCALAR_LOSS_MSE ? (2.0f * e) / den : (e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f)) / den;
        }
        a.dout[k] = seed;
        a.parts[k * 3] = e2;
        a.parts[k * 3 + 1] = ea;
        a.parts[k * 3 + 2] = pres;
    }
}

// (sum over the block's 256 threads, the same tree for every call: xor butterfly inside a wave, then (w0 + w1) + (w2 + w3))
__device__ __forceinline__ float scalar_block_sum(float v, float* red, int tid) {
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// One block: per property, thread i sums the crystals i, i + 256, ... in that order and the block sums the threads with the fixed tree;
// stats[1 + 3 p ..] += sum e^2, sum |e|, present;  stats[0] += sum over p in ascending order of (sum l / count_global[p]) / P
__global__ __launch_bounds__(256) void scalar_stats_kernel(const float* __restrict__ parts, const int* __restrict__ count_global, int B, int P,
                                                           int loss_kind, float* __restrict__ stats) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    float total = 0.f;
    for (int p = 0; p < P; ++p) {
        float s2 = 0.f, sa = 0.f, sn = 0.f;
        for (int b = tid; b < B; b += 256) {
            const float* q = parts + ((size_t)b * P + p) * 3;
            s2 += q[0];
            sa += q[1];
            sn += q[2];
        }
        s2 = scalar_block_sum(s2, red, tid);
        sa = scalar_block_sum(sa, red, tid);
        sn = scalar_block_sum(sn, red, tid);
        if (tid == 0) {
            stats[1 + 3 * p] += s2;
            stats[2 + 3 * p] += sa;
            stats[3 + 3 * p] += sn;
            const int cg = count_global[p];
            if (cg > 0) total += ((loss_kind == MI_SCALAR_LOSS_MSE ? s2 : sa) / (float)cg) / (float)P;
        }
    }
    if (tid == 0) stats[0] += total;
}

// dgf[b][f] = sum_p d_out[b][p] W[p][f], p ascending
__global__ __launch_bounds__(256) void scalar_dgf_kernel(const float* __restrict__ dout, const float* __restrict__ W, float* __restrict__ dgf, int B,
                                                         int H, int P) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)B * H) return;
    const int b = (int)(idx / H), f = (int)(idx % H);
    float s = 0.f;
    for (int p = 0; p < P; ++p) s += dout[(size_t)b * P + p] * W[(size_t)p * H + f];
    dgf[idx] = s;
}

// grad_W[p][f] += sum_b d_out[b][p] gf[b][f] and (threads behind the P H elements of W) grad_bias[p] += sum_b d_out[b][p]: four partial sums
// over the crystals b = k, k + 4, ... in ascending order, combined as (s0 + s1) + (s2 + s3)
__global__ __launch_bounds__(256) void scalar_wgrad_kernel(const float* __restrict__ dout, const float* __restrict__ gf, float* __restrict__ gW,
                                                           float* __restrict__ gb, int B, int H, int P) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, nW = (int64_t)P * H;
    if (idx >= nW + P) return;
    const bool is_w = idx < nW;
    const int p = is_w ? (int)(idx / H) : (int)(idx - nW), f = is_w ? (int)(idx % H) : 0;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b0 = 0; b0 < B; b0 += 4)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int b = b0 + k;
            if (b < B) {
                const float dv = dout[(size_t)b * P + p];
                s[k] += is_w ? dv * gf[(size_t)b * H + f] : dv;
            }
        }
    const float v = (s[0] + s[1]) + (s[2] + s[3]);
    if (is_w) gW[idx] += v;
    else gb[p] += v;
}

// d hf[i][f] = dgf[g(i)][f] / n_g: the graph-mean term of heads_bwd_kernel (backward.hip), alone
__global__ __launch_bounds__(256) void scalar_seed_hf_kernel(const float* __restrict__ dgf, const int* __restrict__ node2graph,
                                                             const int* __restrict__ node_off, float* __restrict__ dhf, int N, int H) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)N * H) return;
    const int i = (int)(idx / H), f = (int)(idx % H);
    const int g = node2graph[i];
    dhf[idx] = dgf[(size_t)g * H + f] / (float)(node_off[g + 1] - node_off[g]);
}

int scalar_seed_hf(const mi_batch* b, const float* dgf, float* dhf, int H, hipStream_t s) {
    const int64_t n = (int64_t)b->N * H;
    if (n == 0) return MI_OK;
    hipLaunchKernelGGL(scalar_seed_hf_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, dgf, b->node2graph, b->node_off, dhf, b->N, H);
    MI_KERNEL_CHECK();
    return MI_OK;
}

// the handle's buffers of these entries, allocated on first use (the per-property ones again when a call brings more properties)
static int scalar_buffers(mi_batch* b, int P, bool forward_only) {
    if (!b->sc_gf) MI_TRY(dev_alloc(b, &b->sc_gf, (size_t)b->B * b->H));
    if (forward_only && !b->sc_in) MI_TRY(dev_alloc(b, &b->sc_in, (size_t)b->B * 9 + (size_t)b->N * (3 + MI_NUM_TYPES)));
    if (P > b->sc_P) {
        if (b->sc_dout) dev_release(b, b->sc_dout);
        if (b->sc_parts) dev_release(b, b->sc_parts);
        b->sc_dout = b->sc_parts = nullptr;
        b->sc_P = 0;
        MI_TRY(dev_alloc(b, &b->sc_dout, (size_t)b->B * P));
        MI_TRY(dev_alloc(b, &b->sc_parts, (size_t)b->B * P * 3));
        b->sc_P = P;
    }
    b->sc_last_P = P;   // (sc_dout and sc_parts are laid out [B][P] of THIS call: mi_scalar_read takes no other P)
    return MI_OK;
}

// the body of the entries (net.h): `what` names the entry in the messages, `stage` replaces the clean-input launch
int scalar_run(const char* what, mi_net* net, mi_batch* b, const float* lengths, const float* angles, const float* frac0, const int* atom_types,
               const float* time_freqs, const int* times, int t_all, const float* W, const float* bias, int P, const float* yhat, const int* have,
               const int* have_host, const int* count_global, const int* count_global_host, int accum_steps, int loss_kind, float* grad_theta,
               float* grad_W, float* grad_bias, float* stats, float* out, void* stream, scalar_input_stage_fn stage, void* stage_ctx, bool own_inputs,
               const float* ig_dout, const InputGradOut* ig) {
    // (ig -- input_grad.hip: the taped forward, dgf = ig_dout W, and the trunk's data-only backward down to the inputs: no loss, no gradient buffer)
    MI_CHECK(!b || !b->pool || pool_stream(b->pool) == (hipStream_t)stream, MI_EINVAL, "%s: a pooled batch handle is used on its pool's stream only", what);
    MI_CHECK(net && b, MI_EINVAL, "null handle");
    MI_CHECK(b->H == net->H && b->L == net->L, MI_EINVAL, "batch was created for a different network");
    MI_CHECK(net->H <= SCALAR_MAX_H, MI_EINVAL, "%s: hidden_dim %d is above %d", what, net->H, SCALAR_MAX_H);
    MI_CHECK(!b->time_map, MI_EINVAL, "%s: the handle carries a time map (the predictor runs on the trained grid)", what);
    MI_CHECK(!b->cond_on && !b->lik_on, MI_EINVAL, "%s: the handle carries a condition or a likelihood mask", what);
    MI_CHECK(!b->gd_on, MI_EINVAL, "%s: the handle carries guidance (mi_batch_clear_guidance first)", what);
    MI_CHECK(b->tape.wcur == 0, MI_EINVAL, "%s: the handle has pending deferred weight gradients (mi_cspnet_wgrad_flush first)", what);
    MI_CHECK(!(grad_theta || ig) || b->tape.wslots == 0, MI_EINVAL, "%s: the handle has an open weight-gradient window (mi_batch_set_wgrad_window(.., 0) first)", what);
    MI_CHECK(P >= 1, MI_EINVAL, "%s: P = %d properties: at least 1", what, P);
    MI_CHECK(accum_steps >= 1, MI_EINVAL, "%s: accum_steps = %d must be >= 1", what, accum_steps);
    MI_CHECK(loss_kind == MI_SCALAR_LOSS_MSE || loss_kind == MI_SCALAR_LOSS_L1, MI_EINVAL, "%s: unknown loss_kind %d", what, loss_kind);
    MI_CHECK(!yhat || (have && have_host && count_global && count_global_host), MI_EINVAL, "%s: yhat without have (and the counts of present targets)", what);
    MI_CHECK(yhat || (!grad_theta && !stats), MI_EINVAL, "%s: a loss (grad_theta, stats) without yhat", what);
    MI_CHECK(!grad_theta || (grad_W && grad_bias), MI_EINVAL, "%s: grad_theta without grad_W and grad_bias", what);
    const int B = b->B, N = b->N, H = net->H;
    if (yhat)
        for (int p = 0; p < P; ++p) {
            int own = 0;
            for (int c = 0; c < B; ++c) {
                const int h = have_host[(size_t)c * P + p];
                MI_CHECK(h == 0 || h == 1, MI_EINVAL, "%s: have[%d][%d] = %d is neither 0 nor 1", what, c, p, h);
                own += h;
            }
            MI_CHECK(count_global_host[p] >= own, MI_EINVAL, "%s: count_global[%d] = %d is below the handle's %d present targets", what, p,
                     count_global_host[p], own);
        }
    if (B == 0 || N == 0) return MI_OK;
    MI_CHECK((stage || (lengths && angles && frac0 && atom_types)) && time_freqs && W && bias, MI_EINVAL, "null argument");
    MI_CHECK(!(grad_theta || ig) || net->W2T != nullptr, MI_ESTATE, "mi_net_set_params must run before backward");
    TraceRange range(what);
    hipStream_t s = (hipStream_t)stream;
    const bool train = grad_theta != nullptr || ig != nullptr;
    if (train) MI_TRY(net_tape_prepare(net, b));
    if (ig) MI_TRY(input_grad_prepare(net, b, s));
    MI_TRY(scalar_buffers(b, P, !train && !own_inputs));
    Tape& tp = b->tape;
    ScalarStageIO io{};
    io.train = train;
    if (!own_inputs) {
        io.w_lat = train ? tp.nz_lat : b->sc_in;
        io.w_frac = train ? tp.nz_frac : b->sc_in + (size_t)B * 9;
        io.w_types = train ? tp.nz_types : b->sc_in + (size_t)B * 9 + (size_t)N * 3;
    }
    io.in_lat = io.w_lat;
    io.in_frac = io.w_frac;
    io.in_types = io.w_types;
    if (stage) {
        MI_TRY(stage(net, b, &io, stage_ctx, s));
    } else {
        ScalarInputArgs ia{lengths, angles, frac0, atom_types, b->node_off, time_freqs, times, t_all, net->TD, io.w_lat, io.w_frac, io.w_types, b->temb};
        hipLaunchKernelGGL(scalar_inputs_kernel, dim3(B), dim3(256), 0, s, ia);
        MI_KERNEL_CHECK();
    }
    const float *in_lat = io.in_lat, *in_frac = io.in_frac, *in_types = io.in_types;
    if (train) {
        tp.borrow_inputs = true;   // (the inputs live in this tape and the time embedding in this batch until the backward below has run)
        const int rc = net_forward(net, b, b->temb, in_types, in_frac, in_lat, nullptr, nullptr, nullptr, s, true, false, false, true);
        tp.borrow_inputs = false;
        MI_TRY(rc);
    } else {
        MI_TRY(net_forward(net, b, b->temb, in_types, in_frac, in_lat, nullptr, nullptr, nullptr, s, false, false, false, true));
    }
    ScalarHeadArgs ha{b->hf, b->node_off, W, bias, yhat, have, count_global, b->sc_gf, out, b->sc_dout, b->sc_parts, H, P, loss_kind, accum_steps};
    hipLaunchKernelGGL(scalar_head_kernel, dim3(B), dim3(256), 0, s, ha);
    if (yhat && stats) hipLaunchKernelGGL(scalar_stats_kernel, dim3(1), dim3(256), 0, s, b->sc_parts, count_global, B, P, loss_kind, stats);
    MI_KERNEL_CHECK();
    if (!train) return MI_OK;
    if (ig) {
        hipLaunchKernelGGL(scalar_dgf_kernel, dim3((unsigned)cdiv((int64_t)B * H, 256)), dim3(256), 0, s, ig_dout, W, tp.dgf, B, H, P);
        MI_KERNEL_CHECK();
        return net_backward(net, b, nullptr, nullptr, nullptr, nullptr, s, tp.dgf, ig);
    }
    hipLaunchKernelGGL(scalar_dgf_kernel, dim3((unsigned)cdiv((int64_t)B * H, 256)), dim3(256), 0, s, b->sc_dout, W, tp.dgf, B, H, P);
    hipLaunchKernelGGL(scalar_wgrad_kernel, dim3((unsigned)cdiv((int64_t)P * H + P, 256)), dim3(256), 0, s, b->sc_dout, b->sc_gf, grad_W, grad_bias, B, H, P);
    MI_KERNEL_CHECK();
    return net_backward(net, b, nullptr, nullptr, nullptr, grad_theta, s, tp.dgf);
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_scalar_forward(mi_net* net, mi_batch* b, const float* lengths, const float* angles, const float* frac0, const int* atom_types,
                      const float* time_freqs, const int* times, int t_all, const float* W, const float* bias, int P, float* out, void* stream) {
    MI_NO_LATENT(net, "mi_scalar_forward");
    MI_CHECK(out, MI_EINVAL, "mi_scalar_forward: null argument");
    return scalar_run("mi_scalar_forward", net, b, lengths, angles, frac0, atom_types, time_freqs, times, t_all, W, bias, P, nullptr, nullptr, nullptr,
                      nullptr, nullptr, 1, MI_SCALAR_LOSS_MSE, nullptr, nullptr, nullptr, nullptr, out, stream);
}

int mi_scalar_micro_step(mi_net* net, mi_batch* b, const float* lengths, const float* angles, const float* frac0, const int* atom_types,
                         const float* time_freqs, const int* times, int t_all, const float* W, const float* bias, int P, const float* yhat,
                         const int* have, const int* have_host, const int* count_global, const int* count_global_host, int accum_steps,
                         int loss_kind, float* grad_theta, float* grad_W, float* grad_bias, float* stats, float* out, void* stream) {
    MI_NO_LATENT(net, "mi_scalar_micro_step");
    return scalar_run("mi_scalar_micro_step", net, b, lengths, angles, frac0, atom_types, time_freqs, times, t_all, W, bias, P, yhat, have, have_host,
                      count_global, count_global_host, accum_steps, loss_kind, grad_theta, grad_W, grad_bias, stats, out, stream);
}

int mi_scalar_read(const mi_batch* b, int P, float* gf, float* d_out, void* stream) {
    MI_CHECK(b, MI_EINVAL, "null handle");
    MI_POOL_STREAM(b, stream, "mi_scalar_read");
    MI_CHECK(b->sc_gf && P >= 1 && P == b->sc_last_P, MI_ESTATE, "mi_scalar_read: the last predictor call on this handle was not one for %d properties", P);
    hipStream_t s = (hipStream_t)stream;
    if (gf && b->B) MI_HIP(hipMemcpyAsync(gf, b->sc_gf, (size_t)b->B * b->H * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (d_out && b->B) MI_HIP(hipMemcpyAsync(d_out, b->sc_dout, (size_t)b->B * P * sizeof(float), hipMemcpyDeviceToDevice, s));
    return MI_OK;
}

}  // extern "C"
