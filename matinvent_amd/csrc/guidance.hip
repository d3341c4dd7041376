// A property-conditioned prior and classifier-free guidance (include/matinvent_hip_guidance.h): the crystal embedding
// [time | property], the condition dropout of the supervised micro-step, and the combination of a conditional and a null evaluation in
// the reverse step.  Three kernels, one thread per element, no atomics:
//   crystal_embedding_kernel   a row's time columns with time_embedding_kernel's (sampler.hip) / time_embedding_mapped_kernel's
//                              (stride.hip) arithmetic, its property columns through csrc/guidance_embed.h, the null row as exact zeros;
//   cond_drop_kernel           one Philox uniform per crystal, indexed by the crystal's position in the whole mini-batch;
//   guidance_combine_kernel    p_c + gamma (p_c - p_u) over the step's prediction arrays, in place.
// Everything is separately rounded: no contraction into FMAs in this unit.
#pragma clang fp contract(off)

#include <cmath>

#include "../../include/matinvent_hip_guidance.h"
#include "net.h"
#include "guidance_embed.h"

namespace mi {

// out[b][c]: c < TD - Z the time part (map != NULL: the time is map[clamp(step)]), else column c - (TD - Z) of the property part.
// on = yhat != NULL && have[b][p] && !(drop && drop[b]); a column that is not on is 0.f.
__global__ __launch_bounds__(256) void crystal_embedding_kernel(const int* __restrict__ map, int n_map, const int* __restrict__ times, int t_all,
                                                                const float* __restrict__ tfreqs, const float* __restrict__ pfreqs,
                                                                const float* __restrict__ yhat, const int* __restrict__ have,
                                                                const int* __restrict__ drop, float* __restrict__ out, int B, int TD, int Z, int F) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)B * TD) return;
    const int b = (int)(idx / TD), c = (int)(idx % TD), tdim = TD - Z, half = tdim / 2;
    if (c < tdim) {
        int t = times ? times[b] : t_all;
        if (map) {
            t = t < 0 ? 0 : (t >= n_map ? n_map - 1 : t);
            t = map[t];
        }
        const float arg = (float)t * tfreqs[c < half ? c : c - half];
        out[idx] = c < half ? sinf(arg) : cosf(arg);
        return;
    }
    int p, k;
    bool cosine;
    guidance_column_index(c - tdim, F, &p, &k, &cosine);
    const int P = Z / (2 * F);
    float v = 0.f;
    if (yhat && have[b * P + p] != 0 && !(drop && drop[b] != 0)) v = guidance_latent_column(yhat[b * P + p], pfreqs[k], cosine);
    out[idx] = v;
}

__global__ __launch_bounds__(256) void cond_drop_kernel(uint64_t seed, uint32_t step, int64_t graph_offset, int B, float p_uncond, int* __restrict__ drop) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= B) return;
    drop[c] = philox_uniform1(seed, step, DRAW_COND_DROP, (uint64_t)(graph_offset + c)) < p_uncond ? 1 : 0;
}

struct CombineArgs {
    float *pl, *px, *pt;
    const float *ul, *ux, *ut;
    int64_t nl, nx, nt;
    float gamma;
};
// element i of [lattice | coordinate | type]: p = p_c + gamma (p_c - p_u); p_c == p_u gives p_c exactly
__global__ __launch_bounds__(256) void guidance_combine_kernel(CombineArgs a) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float* p;
    const float* u;
    if (i < a.nl) {
        p = a.pl, u = a.ul;
    } else if (i < a.nl + a.nx) {
        i -= a.nl, p = a.px, u = a.ux;
    } else if (i < a.nl + a.nx + a.nt) {
        i -= a.nl + a.nx, p = a.pt, u = a.ut;
    } else {
        return;
    }
    const float pc = p[i], d = pc - u[i], g = a.gamma * d;
    p[i] = pc + g;
}

int crystal_embedding(const mi_net* net, const mi_batch* b, int B, const int* times, int t_all, const float* time_freqs, const float* prop_freqs,
                      const float* yhat, const int* have, const int* drop, float* out, hipStream_t s) {
    MI_CHECK(net && time_freqs && out, MI_EINVAL, "crystal embedding: null argument");
    MI_CHECK(net->Z > 0, MI_EINVAL, "crystal embedding: the network has no property part (mi_net_set_latent)");
    MI_CHECK(!yhat || (have && prop_freqs), MI_EINVAL, "crystal embedding: property values need `have` and the frequency table");
    if (B <= 0) return MI_OK;   // (of `b` the time map alone is read: the handle may hold any number of crystals)
    const bool mapped = b && b->time_map;
    hipLaunchKernelGGL(crystal_embedding_kernel, dim3(cdiv((int64_t)B * net->TD, 256)), dim3(256), 0, s, mapped ? (const int*)b->time_map : nullptr,
                       mapped ? (int)b->time_map_h.size() : 0, times, t_all, time_freqs, prop_freqs, yhat, have, drop, out, B, net->TD, net->Z, net->lat_F);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int guidance_combine(float* pl, const float* ul, size_t nl, float* px, const float* ux, size_t nx, float* pt, const float* ut, size_t nt, float gamma,
                     hipStream_t s) {
    const int64_t n = (int64_t)(nl + nx + nt);
    if (n == 0) return MI_OK;
    CombineArgs a{pl, px, pt, ul, ux, ut, (int64_t)nl, (int64_t)nx, (int64_t)nt, gamma};
    hipLaunchKernelGGL(guidance_combine_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int guidance_check(const mi_net* net, const mi_batch* b, bool has_rec, const char* what) {
    if (!b->gd_on) return MI_OK;
    MI_CHECK(net->Z > 0, MI_EINVAL, "%s carries guidance, the network has no property part (mi_net_set_latent)", what);
    MI_CHECK(b->gd_P == net->lat_P && b->gd_F == net->lat_F, MI_EINVAL, "%s carries guidance for P = %d, F = %d; the network has P = %d, F = %d", what,
             b->gd_P, b->gd_F, net->lat_P, net->lat_F);
    MI_CHECK(!has_rec, MI_EINVAL, "%s carries guidance: a record is not taken (the recorded log-probabilities would not be a guided chain's)", what);
    MI_CHECK(!b->lik_on, MI_EINVAL, "%s carries guidance and a likelihood mask", what);
    MI_CHECK(!b->cond_on, MI_EINVAL, "%s carries guidance and a replacement condition", what);
    MI_CHECK(!b->rs_on, MI_EINVAL, "%s carries guidance and resampling", what);
    MI_CHECK(!b->keep_lattice && !b->keep_coords, MI_EINVAL, "%s carries guidance: CSP mode is not taken", what);
    if (b->gd_gamma != 0.f) {
        const mi_batch* q = b->gd_partner;
        MI_CHECK(q && q->num_atoms_h == b->num_atoms_h && q->H == b->H && q->L == b->L, MI_EINVAL, "%s carries guidance without a matching partner handle", what);
        MI_CHECK(!q->gd_on && !q->cond_on && !q->lik_on && !q->rs_on && !q->pool && !q->knn, MI_EINVAL, "%s: the guidance partner carries state of its own", what);
    }
    return MI_OK;
}

struct CondStage {
    const float *prop_freqs, *yhat;
    const int* have;
    float p_uncond;
    uint64_t seed;
    uint32_t step;
};
static int pretrain_cond_stage(mi_net* net, mi_batch* b, const float* time_freqs, void* ctx, hipStream_t s) {
    const CondStage& c = *(const CondStage*)ctx;
    const int* drop = nullptr;
    if (c.yhat && c.p_uncond > 0.f) {   // (p_uncond = 0, or nothing to drop: no draw)
        if (!b->gd_drop) MI_TRY(dev_alloc(b, &b->gd_drop, (size_t)b->B));
        hipLaunchKernelGGL(cond_drop_kernel, dim3(cdiv(b->B, 256)), dim3(256), 0, s, c.seed, c.step, b->graph_offset, b->B, c.p_uncond, b->gd_drop);
        MI_KERNEL_CHECK();
        drop = b->gd_drop;
    }
    return crystal_embedding(net, nullptr, b->B, b->times, 0, time_freqs, c.prop_freqs, c.yhat, c.have, drop, b->temb, s);
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_net_set_latent(mi_net* net, int P, int F) {
    MI_CHECK(net, MI_EINVAL, "null handle");
    if (P == 0) {
        net->Z = net->lat_P = net->lat_F = 0;
        return MI_OK;
    }
    MI_CHECK(P >= 1 && F >= 1 && F <= MI_GUIDANCE_MAX_FREQS, MI_EINVAL, "mi_net_set_latent: P = %d, F = %d: P >= 1 and 1 <= F <= %d", P, F,
             MI_GUIDANCE_MAX_FREQS);
    const int64_t Z = (int64_t)2 * F * P;
    MI_CHECK(net->TD - Z > 0 && (net->TD - Z) % 2 == 0, MI_EINVAL,
             "mi_net_set_latent: Z = 2 F P = %lld of the network's TD = %d embedding columns leaves %lld for the time part, which must be a positive even "
             "number (the products over K = TD ask TD %% 4 == 0 and nothing more: mi_net_create has checked it)",
             (long long)Z, net->TD, (long long)(net->TD - Z));
    net->Z = (int)Z;
    net->lat_P = P;
    net->lat_F = F;
    return MI_OK;
}

int mi_net_latent_dim(const mi_net* net) { return net ? net->Z : 0; }

int mi_crystal_embedding(const mi_net* net, const mi_batch* b, int B, const int* times, int t_all, const float* time_freqs, const float* prop_freqs,
                         const float* yhat, const int* have, const int* drop, float* out, void* stream) {
    MI_CHECK(B >= 0, MI_EINVAL, "B = %d", B);
    return crystal_embedding(net, b, B, times, t_all, time_freqs, prop_freqs, yhat, have, drop, out, (hipStream_t)stream);
}

int mi_guidance_drop_mask(uint64_t seed, uint32_t noise_step, int64_t graph_offset, int B, float p_uncond, int* drop, void* stream) {
    MI_CHECK(drop && B >= 0 && graph_offset >= 0, MI_EINVAL, "bad argument");
    if (B == 0) return MI_OK;
    hipLaunchKernelGGL(cond_drop_kernel, dim3(cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, seed, noise_step, graph_offset, B, p_uncond, drop);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int mi_pretrain_micro_step_cond(mi_net* net, mi_batch* b, const float* lengths, const float* angles, const float* frac0, const int* atom_types,
                                const float* time_freqs, const int* t_host, const int* t_dev, const float* sched_table_dev, int T, uint64_t seed,
                                uint32_t noise_step, const float* rand_l, const float* rand_x, const float* rand_t, float cost_lattice,
                                float cost_coord, float cost_type, int b_global, int n_global, int accum_steps, float* grad_theta, float* stats,
                                float* out_parts, const float* prop_freqs, const float* yhat, const int* have, float p_uncond, void* stream) {
    MI_CHECK(net && net->Z > 0, MI_EINVAL, "mi_pretrain_micro_step_cond: the network has no property part (mi_net_set_latent); mi_pretrain_micro_step trains it");
    MI_CHECK(!yhat || (have && prop_freqs), MI_EINVAL, "mi_pretrain_micro_step_cond: property values need `have` and the frequency table");
    MI_CHECK(p_uncond >= 0.f && p_uncond <= 1.f, MI_EINVAL, "mi_pretrain_micro_step_cond: p_uncond = %g lies outside [0, 1]", (double)p_uncond);
    CondStage ctx{prop_freqs, yhat, have, p_uncond, seed, noise_step};
    return pretrain_micro_run("mi_pretrain_micro_step_cond", net, b, lengths, angles, frac0, atom_types, time_freqs, t_host, t_dev, sched_table_dev, T,
                              seed, noise_step, rand_l, rand_x, rand_t, cost_lattice, cost_coord, cost_type, b_global, n_global, accum_steps, grad_theta,
                              stats, out_parts, pretrain_cond_stage, &ctx, stream);
}

int mi_batch_set_guidance(mi_batch* b, mi_batch* partner, const float* yhat_host, const int* have_host, int P, int F, float gamma) {
    MI_NO_POOLED(b, "mi_batch_set_guidance");
    MI_NO_POOLED(partner, "mi_batch_set_guidance");
    MI_CHECK(b && yhat_host && have_host, MI_EINVAL, "null argument");
    MI_CHECK(P >= 1 && F >= 1 && F <= MI_GUIDANCE_MAX_FREQS, MI_EINVAL, "mi_batch_set_guidance: P = %d, F = %d: P >= 1 and 1 <= F <= %d", P, F,
             MI_GUIDANCE_MAX_FREQS);
    MI_CHECK(std::isfinite(gamma), MI_EINVAL, "mi_batch_set_guidance: gamma is not finite");
    MI_CHECK(!b->knn, MI_EINVAL, "mi_batch_set_guidance: a knn handle is not taken");
    if (gamma != 0.f) {
        MI_CHECK(partner && partner != b, MI_EINVAL, "mi_batch_set_guidance: gamma != 0 needs a partner handle other than the handle itself");
        MI_CHECK(!partner->knn && partner->H == b->H && partner->L == b->L && partner->num_atoms_h == b->num_atoms_h &&
                     partner->node_offset == b->node_offset && partner->graph_offset == b->graph_offset,
                 MI_EINVAL, "mi_batch_set_guidance: the partner handle does not have the handle's network shape, atom counts and offsets");
        MI_CHECK(!partner->gd_on, MI_EINVAL, "mi_batch_set_guidance: the partner handle carries guidance itself");
    }
    for (size_t i = 0; i < (size_t)b->B * P; ++i)
        MI_CHECK(have_host[i] == 0 || std::isfinite(yhat_host[i]), MI_EINVAL, "mi_batch_set_guidance: yhat[%zu] is not finite and have[%zu] != 0", i, i);
    const int need = b->B * P;
    if (!b->gd_freqs) MI_TRY(dev_alloc(b, &b->gd_freqs, (size_t)MI_GUIDANCE_MAX_FREQS));
    if (need > b->gd_cap || !b->gd_yhat) {   // (B is the handle's: the arrays grow only when a later call brings more properties)
        float* yh = nullptr;
        int* hv = nullptr;
        MI_TRY(dev_alloc(b, &yh, (size_t)need));
        MI_TRY(dev_alloc(b, &hv, (size_t)need));
        if (b->gd_yhat) dev_release(b, b->gd_yhat);
        if (b->gd_have) dev_release(b, b->gd_have);
        b->gd_yhat = yh;
        b->gd_have = hv;
        b->gd_cap = need;
    }
    float fr[MI_GUIDANCE_MAX_FREQS] = {0};
    for (int k = 0; k < F; ++k) fr[k] = (float)(3.14159265358979323846 / 8.0 * (double)(1 << k));
    MI_HIP(hipMemcpy(b->gd_freqs, fr, sizeof fr, hipMemcpyHostToDevice));
    if (need > 0) {
        MI_HIP(hipMemcpy(b->gd_yhat, yhat_host, (size_t)need * sizeof(float), hipMemcpyHostToDevice));
        MI_HIP(hipMemcpy(b->gd_have, have_host, (size_t)need * sizeof(int), hipMemcpyHostToDevice));
    }
    b->gd_P = P;
    b->gd_F = F;
    b->gd_gamma = gamma;
    b->gd_partner = gamma != 0.f ? partner : nullptr;
    b->gd_on = true;
    return MI_OK;
}

int mi_batch_clear_guidance(mi_batch* b) {
    MI_CHECK(b, MI_EINVAL, "null handle");
    b->gd_on = false;
    b->gd_partner = nullptr;
    b->gd_gamma = 0.f;
    return MI_OK;
}

int mi_guidance_combine(const float* p_c, const float* p_u, float gamma, int64_t nl, int64_t nx, int64_t nt, float* out, void* stream) {
    MI_CHECK(p_c && p_u && out && nl >= 0 && nx >= 0 && nt >= 0, MI_EINVAL, "bad argument");
    const int64_t n = nl + nx + nt;
    if (n == 0) return MI_OK;
    // (the step's own launch, in place in `out`: its three arrays are the three segments of this one)
    if (out != p_c) MI_HIP(hipMemcpyAsync(out, p_c, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return guidance_combine(out, p_u, (size_t)nl, out + nl, p_u + nl, (size_t)nx, out + nl + nx, p_u + nl + nx, (size_t)nt, gamma, (hipStream_t)stream);
}

}  // extern "C"
