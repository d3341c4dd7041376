// Classifier guidance (include/matinvent_hip_inputgrad.h): the property predictor's INPUT gradient -- the closing launches of
// net_backward's data-only form (backward.hip: `ig`) -- and the guided shift of a chain state.  Launches of this unit, no atomics:
//   ig_pack_wT_kernel    one thread per element: every layer's Fourier columns of edge_mlp.0.weight transposed, [L][6F][H] (gemm_nt's W operand;
//                        once per parameter version);
//   ig_pairs_kernel      one thread per (pair, axis): dDelta (=, += over the layers) sum_k w_k (dS cos(w_k Delta) - dC sin(w_k Delta)), k ascending,
//                        with fourier_kernel's own argument arithmetic (cspnet.hip: pymod1 of the difference, (float)k * 2 pi, sincos_bounded);
//   ig_scatter_kernel    one block per crystal, one atom per thread: the atom's pairs in ascending pair order, g_frac[j] += dDelta, g_frac[i] -= dDelta;
//   ig_lattice_kernel    one block per crystal: M = sum_l dG_l W_l[:, 2H .. 2H + 9) (layers L - 1 ... 0, columns in a fixed tree), then (M + M^T) L;
//   ig_types_kernel      one thread per (atom, type): dXa node_embedding.weight, c ascending;
//   guide_seed_kernel    one thread per crystal;   guide_shift_kernel   one block per crystal (csrc/guide_shift.h).
// The contraction order of g_frac: FIRST the library's product [dS | dC] = [Dm Wsin | Dp Wcos] on the pass's fp32 rows (gemm_nt), THEN the
// chain rule through sin / cos -- not [derivative features] W^T row-dotted with Dm / Dp, whose product is H wide instead of 6F.

#include <cmath>

#include "../../include/matinvent_hip_inputgrad.h"
#include "net.h"
#include "guide_shift.h"

namespace mi {

extern int g_edge_pairs;   // cspnet.hip (mi_set_edge_pairs)

static_assert(GUIDE_MODE_MAX == MI_GUIDE_MODE_MAX && GUIDE_MODE_MIN == MI_GUIDE_MODE_MIN && GUIDE_MODE_TARGET == MI_GUIDE_MODE_TARGET, "modes");

// wT[l][k][c] = theta[w0 + l stride + c edge_in + 2H + 9 + k],  k < 6F, c < H
__global__ __launch_bounds__(256) void ig_pack_wT_kernel(const float* __restrict__ theta, int64_t w0, int64_t stride, int edge_in, int H, int F6, int L,
                                                         float* __restrict__ wT) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)L * F6 * H) return;
    const int c = (int)(idx % H), k = (int)((idx / H) % F6), l = (int)(idx / ((int64_t)H * F6));
    wT[idx] = theta[w0 + (int64_t)l * stride + (int64_t)c * edge_in + 2 * H + 9 + k];
}

// dSC [Np][6F] = [dS (3F) | dC (3F)], columns d F + k as the features'.  d sin(w D) / dD = w cos(w D), d cos(w D) / dD = -w sin(w D); `% 1` has slope 1.
__global__ __launch_bounds__(256) void ig_pairs_kernel(const float* __restrict__ frac, const int* __restrict__ pair_i, const int* __restrict__ pair_j,
                                                       const float* __restrict__ dSC, float* __restrict__ dd, int64_t Np, int F, int first) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= Np * 3) return;
    const int64_t p = idx / 3;
    const int d = (int)(idx % 3);
    const float delta = pymod1(frac[pair_j[p] * 3 + d] - frac[pair_i[p] * 3 + d]);
    const float* dS = dSC + p * (6 * F) + d * F;
    const float* dC = dS + 3 * F;
    float acc = 0.f;
    for (int k = 0; k < F; ++k) {
        const float w = (float)k * 6.28318530717958647692f;
        float sn, cs;
        sincos_bounded(delta * w, &sn, &cs);
        acc += w * (dS[k] * cs - dC[k] * sn);
    }
    dd[idx] = first ? acc : dd[idx] + acc;
}

// Pair (i < j) of a crystal of n atoms is row pair_off[g] + i n - i (i + 1) / 2 + (j - i - 1) (the fc pair list's order).  Atom a: the pairs
// (i, a), i < a, come first in that order -- it is their j: += -- then the pairs (a, j), j > a -- it is their i: -=.
__global__ __launch_bounds__(256) void ig_scatter_kernel(const float* __restrict__ dd, const int* __restrict__ node_off, const int* __restrict__ pair_off,
                                                         float* __restrict__ g_frac) {
    const int g = blockIdx.x;
    const int o = node_off[g], n = node_off[g + 1] - o;
    const int64_t p0 = pair_off[g];
    for (int a = threadIdx.x; a < n; a += 256) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int i = 0; i < a; ++i) {
            const float* r = dd + (p0 + (int64_t)i * n - (int64_t)i * (i + 1) / 2 + (a - i - 1)) * 3;
            s0 += r[0];
            s1 += r[1];
            s2 += r[2];
        }
        const int64_t row = p0 + (int64_t)a * n - (int64_t)a * (a + 1) / 2;
        for (int j = a + 1; j < n; ++j) {
            const float* r = dd + (row + (j - a - 1)) * 3;
            s0 -= r[0];
            s1 -= r[1];
            s2 -= r[2];
        }
        float* out = g_frac + (size_t)(o + a) * 3;
        out[0] = s0;
        out[1] = s1;
        out[2] = s2;
    }
}

// thread t sums the columns c = t, t + 256, ... of every layer (l = L - 1 ... 0, c ascending), then the block's fixed tree; lattice_ips = L L^T
// (row a of L times row b): d / dL[a][k] = sum_b (M[a][b] + M[b][a]) L[b][k]
__global__ __launch_bounds__(256) void ig_lattice_kernel(const float* __restrict__ dG, const float* __restrict__ theta, int64_t w0, int64_t stride,
                                                         int edge_in, int H, int L, int B, const float* __restrict__ lattices, float* __restrict__ g_lat) {
    __shared__ float red[9][4];
    __shared__ float M[9];
    const int b = blockIdx.x, tid = threadIdx.x;
    float acc[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) acc[q] = 0.f;
    for (int l = L - 1; l >= 0; --l) {
        const float* dg = dG + ((size_t)l * B + b) * H;
        const float* w = theta + w0 + (int64_t)l * stride + 2 * H;
        for (int c = tid; c < H; c += 256) {
            const float v = dg[c];
#pragma unroll
            for (int q = 0; q < 9; ++q) acc[q] += v * w[(int64_t)c * edge_in + q];
        }
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        const float v = wave_sum(acc[q]);
        if ((tid & 63) == 0) red[q][tid >> 6] = v;
    }
    __syncthreads();
    if (tid < 9) M[tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
    __syncthreads();
    if (tid < 9) {
        const int a = tid / 3, k = tid % 3;
        const float* Lm = lattices + (size_t)b * 9;
        float s = 0.f;
#pragma unroll
        for (int bb = 0; bb < 3; ++bb) s += (M[a * 3 + bb] + M[bb * 3 + a]) * Lm[bb * 3 + k];
        g_lat[(size_t)b * 9 + tid] = s;
    }
}

// g_types[i][k] = sum_c dXa[i][c] Wemb[c][k]   (node_embedding.weight [H][100])
__global__ __launch_bounds__(256) void ig_types_kernel(const float* __restrict__ dXa, const float* __restrict__ Wemb, float* __restrict__ g_types, int N,
                                                       int H) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)N * MI_NUM_TYPES) return;
    const int i = (int)(idx / MI_NUM_TYPES), k = (int)(idx % MI_NUM_TYPES);
    const float* x = dXa + (size_t)i * H;
    float s = 0.f;
    for (int c = 0; c < H; ++c) s += x[c] * Wemb[(size_t)c * MI_NUM_TYPES + k];
    g_types[idx] = s;
}

__global__ __launch_bounds__(256) void guide_seed_kernel(const float* __restrict__ out, int B, int P, int p, int mode, float target_hat,
                                                         float* __restrict__ d_out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float o = out[(size_t)b * P + p];
    const float v = guide_finite(o) ? guide_seed(o, mode, target_hat) : 0.f;
    for (int q = 0; q < P; ++q) d_out[(size_t)b * P + q] = q == p ? v : 0.f;
}

struct GuideShiftArgs {
    const int* node_off;
    float *types, *frac, *lat;
    const float *g_types, *g_frac, *g_lat;
    float a_t, a_x, a_l, max_shift;
};
// One block per crystal: every thread scans its share of the crystal's gradient elements, the block agrees on "all finite" (uniform), and only
// then anything of the crystal is written.
__global__ __launch_bounds__(256) void guide_shift_kernel(GuideShiftArgs a) {
    __shared__ int bad_s[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n0 = a.node_off[b], n = a.node_off[b + 1] - n0;
    const float* gl = a.g_lat + (size_t)b * 9;
    const float* gx = a.g_frac + (size_t)n0 * 3;
    const float* gt = a.g_types ? a.g_types + (size_t)n0 * MI_NUM_TYPES : nullptr;
    int bad = 0;
    if (tid < 9 && !guide_finite(gl[tid])) bad = 1;
    for (int i = tid; i < n * 3; i += 256)
        if (!guide_finite(gx[i])) bad = 1;
    if (gt)
        for (int i = tid; i < n * MI_NUM_TYPES; i += 256)
            if (!guide_finite(gt[i])) bad = 1;
    bad = __any(bad) ? 1 : 0;
    if ((tid & 63) == 0) bad_s[tid >> 6] = bad;
    __syncthreads();
    if (bad_s[0] | bad_s[1] | bad_s[2] | bad_s[3]) return;   // (uniform over the block)
    float* lat = a.lat + (size_t)b * 9;
    float* x = a.frac + (size_t)n0 * 3;
    if (tid < 9) lat[tid] = guide_shift_plain(lat[tid], a.a_l, gl[tid], a.max_shift);
    for (int i = tid; i < n * 3; i += 256) x[i] = guide_shift_wrapped(x[i], a.a_x, gx[i], a.max_shift);
    if (gt) {
        float* ty = a.types + (size_t)n0 * MI_NUM_TYPES;
        for (int i = tid; i < n * MI_NUM_TYPES; i += 256) ty[i] = guide_shift_plain(ty[i], a.a_t, gt[i], a.max_shift);
    }
}

// the parameter block of every layer has one size: a constant stride between the layers' edge_mlp.0.weight (checked)
static int layer_stride(const mi_net* net, int64_t* w0, int64_t* stride) {
    *w0 = net->off("csp_layer_0.edge_mlp.0.weight");
    *stride = net->L >= 2 ? net->off("csp_layer_1.edge_mlp.0.weight") - *w0 : 0;
    for (int l = 2; l < net->L; ++l)
        MI_CHECK(net->off("csp_layer_" + std::to_string(l) + ".edge_mlp.0.weight") == *w0 + l * *stride, MI_EINVAL,
                 "input gradient: the layers' parameter blocks differ in size");
    return MI_OK;
}

int input_grad_prepare(mi_net* net, mi_batch* b, hipStream_t s) {
    const int H = net->H, L = net->L, F6 = 6 * net->F;
    if (!b->ig_dd) MI_TRY(dev_alloc(b, &b->ig_dd, (size_t)std::max<int64_t>(b->Np, 1) * 3));
    if (!b->ig_wT) MI_TRY(dev_alloc(b, &b->ig_wT, (size_t)L * F6 * H));
    if (b->ig_net == (const void*)net && b->ig_epoch == net->param_epoch) return MI_OK;
    int64_t w0, stride;
    MI_TRY(layer_stride(net, &w0, &stride));
    hipLaunchKernelGGL(ig_pack_wT_kernel, dim3((unsigned)cdiv((int64_t)L * F6 * H, 256)), dim3(256), 0, s, net->theta, w0, stride, net->edge_in, H, F6, L,
                       b->ig_wT);
    MI_KERNEL_CHECK();
    b->ig_net = net;
    b->ig_epoch = net->param_epoch;
    return MI_OK;
}

int input_grad_pairs(mi_net* net, mi_batch* b, const float* frac, const float* dSC, bool first, hipStream_t s) {
    if (b->Np == 0) return MI_OK;
    hipLaunchKernelGGL(ig_pairs_kernel, dim3((unsigned)cdiv(b->Np * 3, 256)), dim3(256), 0, s, frac, b->pair_i, b->pair_j, dSC, b->ig_dd, b->Np, net->F,
                       first ? 1 : 0);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int input_grad_finish(mi_net* net, mi_batch* b, const InputGradOut* ig, const float* lattices, const float* dG, const float* dXa, hipStream_t s) {
    const int B = b->B, N = b->N, H = net->H;
    int64_t w0, stride;
    MI_TRY(layer_stride(net, &w0, &stride));
    hipLaunchKernelGGL(ig_scatter_kernel, dim3(B), dim3(256), 0, s, b->ig_dd, b->node_off, b->pair_off, ig->g_frac);
    hipLaunchKernelGGL(ig_lattice_kernel, dim3(B), dim3(256), 0, s, dG, net->theta, w0, stride, net->edge_in, H, net->L, B, lattices, ig->g_lat);
    if (ig->g_types)
        hipLaunchKernelGGL(ig_types_kernel, dim3((unsigned)cdiv((int64_t)N * MI_NUM_TYPES, 256)), dim3(256), 0, s, dXa, net->p("node_embedding.weight"),
                           ig->g_types, N, H);
    MI_KERNEL_CHECK();
    return MI_OK;
}

// the refusals below that need no launch, under a caller's name (net.h): mi_scalar_input_grad's knn, pair-mode and window lines, then
// scalar_run's (scalar_head.hip) network / batch mismatch, time map, condition or likelihood mask, guidance, pending weight gradients and
// W2T lines, in the order the two raise them.  Those stay the source of truth; a refusal added there belongs here too.
int input_grad_refusals(const char* what, const mi_net* net, const mi_batch* b) {
    MI_CHECK(!b->knn, MI_EINVAL, "%s: a knn-style handle (the input gradient runs in the fully connected pair mode only)", what);
    MI_CHECK(g_edge_pairs && net->H % 4 == 0, MI_EINVAL, "%s: pair mode is off or hidden_dim %% 4 != 0 (the input gradient runs in pair mode only)", what);
    MI_CHECK(b->tape.wslots == 0, MI_EINVAL, "%s: the handle has an open weight-gradient window (mi_batch_set_wgrad_window(.., 0) first)", what);
    MI_CHECK(b->H == net->H && b->L == net->L, MI_EINVAL, "%s: batch was created for a different network", what);
    MI_CHECK(!b->time_map, MI_EINVAL, "%s: the handle carries a time map (the predictor runs on the trained grid)", what);
    MI_CHECK(!b->cond_on && !b->lik_on, MI_EINVAL, "%s: the handle carries a condition or a likelihood mask", what);
    MI_CHECK(!b->gd_on, MI_EINVAL, "%s: the handle carries guidance (mi_batch_clear_guidance first)", what);
    MI_CHECK(b->tape.wcur == 0, MI_EINVAL, "%s: the handle has pending deferred weight gradients (mi_cspnet_wgrad_flush first)", what);
    MI_CHECK(net->W2T != nullptr, MI_ESTATE, "%s: mi_net_set_params must run before backward", what);
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_scalar_input_grad(mi_net* net, mi_batch* b, const float* atom_types, const float* frac, const float* lattices, const float* time_freqs,
                         const int* times, int t_all, const float* W, const float* bias, int P, const float* d_out, float* out, float* g_types,
                         float* g_frac, float* g_lat, void* stream) {
    const char* what = "mi_scalar_input_grad";
    MI_NO_LATENT(net, "mi_scalar_input_grad");
    MI_NO_POOLED(b, "mi_scalar_input_grad");
    MI_CHECK(!b || !b->knn, MI_EINVAL, "%s: a knn-style handle (the input gradient runs in the fully connected pair mode only)", what);
    MI_CHECK(!net || (g_edge_pairs && net->H % 4 == 0), MI_EINVAL, "%s: pair mode is off or hidden_dim %% 4 != 0 (the input gradient runs in pair mode only)", what);
    MI_CHECK(!b || b->tape.wslots == 0, MI_EINVAL, "%s: the handle has an open weight-gradient window (mi_batch_set_wgrad_window(.., 0) first)", what);
    MI_CHECK(d_out && out && g_frac && g_lat, MI_EINVAL, "%s: null argument", what);
    MI_CHECK(!b || b->B == 0 || b->N == 0 || (atom_types && frac && lattices), MI_EINVAL, "%s: null argument", what);
    ScalarStateCtx ctx{atom_types, frac, lattices, time_freqs, times, t_all};
    InputGradOut ig{g_types, g_frac, g_lat};
    return scalar_run(what, net, b, nullptr, nullptr, nullptr, nullptr, time_freqs, times, t_all, W, bias, P, nullptr, nullptr, nullptr, nullptr, nullptr, 1,
                      MI_SCALAR_LOSS_MSE, nullptr, nullptr, nullptr, nullptr, out, stream, scalar_state_stage, &ctx, true, d_out, &ig);
}

int mi_guide_seed(const float* out, int B, int P, int p, int mode, float target_hat, float* d_out, void* stream) {
    const char* what = "mi_guide_seed";
    MI_CHECK(B >= 0, MI_EINVAL, "%s: B = %d", what, B);
    MI_CHECK(P >= 1 && p >= 0 && p < P, MI_EINVAL, "%s: property p = %d of P = %d", what, p, P);
    MI_CHECK(mode == MI_GUIDE_MODE_MAX || mode == MI_GUIDE_MODE_MIN || mode == MI_GUIDE_MODE_TARGET, MI_EINVAL, "%s: unknown mode %d", what, mode);
    MI_CHECK(mode != MI_GUIDE_MODE_TARGET || std::isfinite(target_hat), MI_EINVAL, "%s: target_hat is not finite", what);
    if (B == 0) return MI_OK;
    MI_CHECK(out && d_out, MI_EINVAL, "%s: null argument", what);
    hipLaunchKernelGGL(guide_seed_kernel, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, out, B, P, p, mode, target_hat, d_out);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int mi_guide_shift(mi_batch* b, float* atom_types, float* frac, float* lattices, const float* g_types, const float* g_frac, const float* g_lat,
                   float a_t, float a_x, float a_l, float max_shift, void* stream) {
    const char* what = "mi_guide_shift";
    MI_CHECK(b, MI_EINVAL, "null handle");
    MI_POOL_STREAM(b, stream, "mi_guide_shift");
    MI_CHECK(std::isfinite(a_t) && std::isfinite(a_x) && std::isfinite(a_l), MI_EINVAL, "%s: a coefficient is not finite", what);
    MI_CHECK(std::isfinite(max_shift), MI_EINVAL, "%s: max_shift is not finite", what);
    if (b->B == 0 || b->N == 0) return MI_OK;
    MI_CHECK(frac && lattices && g_frac && g_lat && (!g_types || atom_types), MI_EINVAL, "%s: null argument", what);
    GuideShiftArgs a{b->node_off, atom_types, frac, lattices, g_types, g_frac, g_lat, a_t, a_x, a_l, max_shift};
    hipLaunchKernelGGL(guide_shift_kernel, dim3(b->B), dim3(256), 0, (hipStream_t)stream, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // extern "C"
