// Replacement conditioning of the reverse chain (include/matinvent_hip_cond.h): a batch handle's condition -- which atom
// types, coordinates and lattices are known, and their clean values -- and the one kernel that imposes it on a state at a noise level.
//
// The arithmetic is add_noise's (diffusion.py:90-113), separately rounded like the sampler's updates: no contraction here either.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>

#include "../../include/matinvent_hip_cond.h"
#include "../../include/matinvent_hip_lik.h"
#include "net.h"
#include "logprob.h"

namespace mi {

struct ConditionArgs {
    const int *known_types, *known_coords, *known_lattice, *types0;   // [N], [N], [B], [N]
    const float *frac0, *lat0;                                        // [N][3], [B][9]
    const float* table;                                               // [levels][3] = (c0, c1, sigma)
    const int* node_off;                                              // [B + 1]
    float *atom_types, *frac, *lattices;                              // the state, known elements overwritten in place
    float *rec_types, *rec_frac, *rec_lat;                            // the record slices of this level, or NULL
    uint64_t seed;
    int64_t node_offset, graph_offset;
    int level;
};

// One 256-thread block per crystal, in the shape of predictor_kernel: the lattice on threads 0..8, the coordinates strided over the block,
// the type rows one wave per atom with a lane owning a quad of logits = one Philox call.  Elements that are not known are skipped before
// anything of theirs is read or drawn.  Level 0: the clean values themselves, the table is not read.
__global__ __launch_bounds__(256) void condition_impose_kernel(ConditionArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int level = a.level;
    const bool noisy = level > 0;
    float c0 = 1.f, c1 = 0.f, sigma = 0.f;
    if (noisy) {
        c0 = a.table[level * 3 + 0];
        c1 = a.table[level * 3 + 1];
        sigma = a.table[level * 3 + 2];
    }
    const int n0 = a.node_off[b], n1 = a.node_off[b + 1];

    // lattice: l = c0 l0 + c1 z
    if (tid < 9 && a.known_lattice && a.known_lattice[b]) {
        const int idx = b * 9 + tid;
        float v = a.lat0[idx];
        if (noisy) {
            const float z = philox_normal1(a.seed, (uint32_t)level, DRAW_COND_L, (uint64_t)a.graph_offset * 9 + idx);
            v = c0 * v + c1 * z;
        }
        a.lattices[idx] = v;
        if (a.rec_lat) a.rec_lat[idx] = v;
    }

    // coordinates: x = (x0 + sigma z) % 1, wrapped twice like the predictor's (the first wrap of a tiny negative value rounds to 1.0)
    if (a.known_coords) {
        for (int idx = n0 * 3 + tid; idx < n1 * 3; idx += 256) {
            if (!a.known_coords[idx / 3]) continue;
            float v = a.frac0[idx];
            if (noisy) {
                const float z = philox_normal1(a.seed, (uint32_t)level, DRAW_COND_X, (uint64_t)a.node_offset * 3 + idx);
                v = v + sigma * z;
            }
            v = pymod1(pymod1(v));
            a.frac[idx] = v;
            if (a.rec_frac) a.rec_frac[idx] = v;
        }
    }

    // atom-type logits: a = c0 onehot + c1 z
    if (a.known_types) {
        for (int i = n0 + wave; i < n1; i += 4) {
            if (!a.known_types[i] || lane >= MI_NUM_TYPES / 4) continue;
            const int64_t idx0 = (int64_t)i * MI_NUM_TYPES + 4 * lane;
            const int hot = a.types0[i] - 1 - 4 * lane;   // the quad's column of the one-hot 1, when in 0..3
            float z[4] = {0.f, 0.f, 0.f, 0.f};
            if (noisy) philox_normal4(a.seed, (uint32_t)level, DRAW_COND_T, ((uint64_t)a.node_offset * MI_NUM_TYPES + idx0) >> 2, z);
            f32x4 vout;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float oh = q == hot ? 1.0f : 0.0f;
                vout[q] = noisy ? c0 * oh + c1 * z[q] : oh;
            }
            *reinterpret_cast<f32x4*>(a.atom_types + idx0) = vout;
            if (a.rec_types) *reinterpret_cast<f32x4*>(a.rec_types + idx0) = vout;
        }
    }
}

int condition_check(const mi_batch* b, int T, const char* what) {
    if (!b->cond_on) return MI_OK;
    MI_CHECK(!b->keep_lattice && !b->keep_coords, MI_EINVAL,
             "%s carries a condition AND CSP mode (keep_lattice / keep_coords): give the known lattice / coordinates through the condition", what);
    MI_CHECK(b->cond_levels == T + 1, MI_EINVAL, "%s carries a condition whose level table has %d rows, the call has T + 1 = %d", what,
             b->cond_levels, T + 1);
    return MI_OK;
}

int condition_impose(const mi_batch* b, int level, uint64_t seed, float* atom_types, float* frac, float* lattices, float* rec_types, float* rec_frac,
                     float* rec_lat, hipStream_t s) {
    MI_CHECK(b->cond_on, MI_EINVAL, "the batch handle carries no condition");
    MI_CHECK(level >= 0 && level < b->cond_levels, MI_EINVAL, "level %d outside the condition's table (0..%d)", level, b->cond_levels - 1);
    if (!b->cond_any || b->B == 0 || b->N == 0) return MI_OK;
    ConditionArgs a;
    a.known_types = b->cond_kt;
    a.known_coords = b->cond_kx;
    a.known_lattice = b->cond_kl;
    a.types0 = b->cond_types0;
    a.frac0 = b->cond_frac0;
    a.lat0 = b->cond_lat0;
    a.table = b->cond_table;
    a.node_off = b->node_off;
    a.atom_types = atom_types;
    a.frac = frac;
    a.lattices = lattices;
    a.rec_types = rec_types;
    a.rec_frac = rec_frac;
    a.rec_lat = rec_lat;
    a.seed = seed;
    a.node_offset = b->node_offset;
    a.graph_offset = b->graph_offset;
    a.level = level;
    hipLaunchKernelGGL(condition_impose_kernel, dim3(b->B), dim3(256), 0, s, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

// predictor_kernel for a recording chain on a handle with a condition AND a likelihood mask: the elements the imposition is about to
// overwrite leave the three recorded log-probabilities.  The state update, the divisors and every free element's arithmetic are
// predictor_kernel's (sampler.hip), line for line -- a kernel of its own, in this unit, so that predictor_kernel's device code stays what
// it was.
__global__ __launch_bounds__(256) void predictor_masked_kernel(PredictorArgs a, LikMask m) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = a.t;
    const StepCoef c = load_coef(a.coef, t);
    const int n0 = a.node_off[b], n1 = a.node_off[b + 1], n = n1 - n0;
    const float cnt = (float)(n > 0 ? n : 1);
    // the three log-probabilities of the step (diffusion.py:357-368) exist for a recording caller only: without one their arithmetic (21 exponentials per
    // coordinate, a logarithm per logit) and block reductions are skipped -- the state update is the same instructions either way
    const bool want_lp = t > 1 && (a.rec_lpl != nullptr || a.rec_lpt != nullptr || a.rec_lpx != nullptr);

    // lattice: l_{t-1} = c0 (l_t - c1 pred_l) + sigma z
    float lp_l = 0.f;
    if (tid < 9) {
        int idx = b * 9 + tid;
        float z = 0.f;
        if (t > 1) z = a.noise_l ? a.noise_l[idx] : philox_normal1(a.seed, (uint32_t)t, DRAW_PRED_L, (uint64_t)a.graph_offset * 9 + idx);
        float mu = c.c0 * (a.lattices[idx] - c.c1 * a.pred_l[idx]);
        float v = a.keep_lattice ? a.lattices[idx] : mu + c.sigma * z;
        a.lattices[idx] = v;
        if (a.rec_lat) a.rec_lat[idx] = v;
        if (want_lp && !m.known_lattice[b]) lp_l = normal_log_prob(v, mu, c.sigma_sq, c.log_sigma);
    }
    if (want_lp) lp_l = block_sum_256(lp_l, red);

    // coordinates: x_{t-1} = (x_{t-1/2} - step * s + std z) % 1
    float lp_x = 0.f;
    for (int idx = n0 * 3 + tid; idx < n1 * 3; idx += 256) {
        float z = 0.f;
        if (t > 1) z = a.noise_x ? a.noise_x[idx] : philox_normal1(a.seed, (uint32_t)t, DRAW_PRED_X, (uint64_t)a.node_offset * 3 + idx);
        float px = a.pred_x[idx] * c.sqrt_sn;
        float drift = a.x_mid[idx] - c.step_pred * px;
        float v = pymod1(a.keep_coords ? a.x_mid[idx] : drift + c.std_pred * z);
        if (want_lp && !m.known_coords[idx / 3]) lp_x += log_prob_wn(v, pymod1(drift), c.std_pred_sq);
        v = pymod1(v);  // traj[t-1]['frac_coords'] = x_{t-1} % 1  (:386)
        a.frac[idx] = v;
        if (a.rec_frac) a.rec_frac[idx] = v;
    }
    if (want_lp) lp_x = block_sum_256(lp_x, red);

    // atom-type logits: one wave per atom; a lane owns a QUAD of consecutive logits = one Philox call (100 logits = 25 quads, and the
    // global element index of a logit row starts at a multiple of 4), instead of one call -- four Box-Muller normals -- per logit
    float lp_t = 0.f;
    for (int i = n0 + wave; i < n1; i += 4) {
        float s = 0.f;
        if (lane < MI_NUM_TYPES / 4) {
            const int64_t idx0 = (int64_t)i * MI_NUM_TYPES + 4 * lane;
            float z[4] = {0.f, 0.f, 0.f, 0.f};
            if (t > 1) {
                if (a.noise_t) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) z[q] = a.noise_t[idx0 + q];
                } else {
                    philox_normal4(a.seed, (uint32_t)t, DRAW_PRED_T, ((uint64_t)a.node_offset * MI_NUM_TYPES + idx0) >> 2, z);
                }
            }
            const f32x4 at = *reinterpret_cast<const f32x4*>(a.atom_types + idx0), pt = *reinterpret_cast<const f32x4*>(a.pred_t + idx0);
            f32x4 vout;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float mu = c.c0 * (at[q] - c.c1 * pt[q]);
                const float v = mu + c.sigma * z[q];
                vout[q] = v;
                if (want_lp && !m.known_types[i]) s += normal_log_prob(v, mu, c.sigma_sq, c.log_sigma);
            }
            *reinterpret_cast<f32x4*>(a.atom_types + idx0) = vout;
            if (a.rec_types) *reinterpret_cast<f32x4*>(a.rec_types + idx0) = vout;
        }
        if (want_lp) {   // (a masked row arrives with s = 0.f and leaves lp_t's bits as they are)
            s = wave_sum(s);
            lp_t += s / (float)MI_NUM_TYPES;  // mean over the 100 logits (:358)
        }
    }
    if (!want_lp) return;
    // every lane of a wave holds the same lp_t; add the four waves
    __syncthreads();
    if (lane == 0) red[wave] = lp_t;
    __syncthreads();
    if (tid == 0 && t > 1) {
        float lpt = ((red[0] + red[1]) + (red[2] + red[3])) / cnt;
        if (a.rec_lpl) a.rec_lpl[b] = (lp_l / 3.0f) / 3.0f;  // .mean(-1).mean(-1) (:357)
        if (a.rec_lpt) a.rec_lpt[b] = lpt;
        if (a.rec_lpx) a.rec_lpx[b] = a.lp_corr[b] + (lp_x / 3.0f) / cnt;
    }
}

int predictor_masked_launch(const mi_batch* b, const PredictorArgs& a, hipStream_t s) {
    MI_CHECK(b->lik_on && b->lik_kt && b->lik_kx && b->lik_kl, MI_ESTATE, "the batch handle carries no likelihood mask");
    hipLaunchKernelGGL(predictor_masked_kernel, dim3(b->B), dim3(256), 0, s, a, LikMask{b->lik_kt, b->lik_kx, b->lik_kl});
    MI_KERNEL_CHECK();
    return MI_OK;
}

int likelihood_mask_same(const mi_batch* p, const mi_batch* q, const char* what) {
    MI_CHECK(p->lik_on == q->lik_on && (!p->lik_on || p->lik_h == q->lik_h), MI_EINVAL, "%s", what);
    return MI_OK;
}

}  // namespace mi

using namespace mi;

namespace {
bool any_set(const int* m, int n) {
    if (!m) return false;
    for (int i = 0; i < n; ++i)
        if (m[i]) return true;
    return false;
}

template <typename T>
int upload(mi_batch* b, T** dev, const T* host, size_t n) {
    if (!*dev) MI_TRY(dev_alloc(b, dev, n));
    if (n) MI_HIP(hipMemcpy(*dev, host, n * sizeof(T), hipMemcpyHostToDevice));
    return MI_OK;
}
}  // namespace

extern "C" {

int mi_batch_set_condition(mi_batch* b, const mi_condition* cond, const float* level_table_host, int n) {
    MI_NO_POOLED(b, "mi_batch_set_condition");
    MI_CHECK(b, MI_EINVAL, "null handle");
    if (!cond) {
        b->cond_on = b->cond_any = b->cond_has_x = b->cond_has_l = false;
        b->cond_levels = 0;
        return MI_OK;
    }
    // every check first: a refused call leaves the handle as it was
    MI_CHECK(level_table_host && n >= 2, MI_EINVAL, "a condition needs a level table of T + 1 >= 2 rows (n = %d)", n);
    for (int k = 0; k < 3 * n; ++k) MI_CHECK(std::isfinite(level_table_host[k]), MI_EINVAL, "level table: row %d holds a non-finite value", k / 3);
    const int N = b->N, B = b->B;
    const bool kt = any_set(cond->known_types_host, N), kx = any_set(cond->known_coords_host, N), kl = any_set(cond->known_lattice_host, B);
    MI_CHECK(!kt || cond->types0_host, MI_EINVAL, "known atom types without types0");
    MI_CHECK(!kx || cond->frac0_host, MI_EINVAL, "known coordinates without frac0");
    MI_CHECK(!kl || cond->lat0_host, MI_EINVAL, "known lattices without lat0");
    if (kt)
        for (int i = 0; i < N; ++i)
            MI_CHECK(!cond->known_types_host[i] || (cond->types0_host[i] >= 1 && cond->types0_host[i] <= MI_NUM_TYPES), MI_EINVAL,
                     "known atom %d has type %d: must be an atomic number 1..%d", i, cond->types0_host[i], MI_NUM_TYPES);
    if (kx)
        for (int i = 0; i < 3 * N; ++i)
            MI_CHECK(!cond->known_coords_host[i / 3] || std::isfinite(cond->frac0_host[i]), MI_EINVAL, "known atom %d has a non-finite coordinate", i / 3);
    if (kl)
        for (int i = 0; i < 9 * B; ++i)
            MI_CHECK(!cond->known_lattice_host[i / 9] || std::isfinite(cond->lat0_host[i]), MI_EINVAL, "known lattice %d has a non-finite entry", i / 9);

    b->cond_on = b->cond_any = b->cond_has_x = b->cond_has_l = false;   // (a failed copy below leaves no half-written condition attached)
    b->cond_levels = 0;
    // parts with nothing known keep a NULL-mask meaning for the kernel: their arrays are not uploaded and not read
    std::vector<int> zeros;
    auto mask = [&](const int* m, int len) -> const int* {
        if (m) return m;
        zeros.assign((size_t)len, 0);
        return zeros.data();
    };
    MI_TRY(upload(b, &b->cond_kt, mask(cond->known_types_host, N), (size_t)N));
    MI_TRY(upload(b, &b->cond_kx, mask(cond->known_coords_host, N), (size_t)N));
    MI_TRY(upload(b, &b->cond_kl, mask(cond->known_lattice_host, B), (size_t)B));
    if (kt) {
        // types of atoms that are not known are never read on the device; upload a checked copy so that a stray value cannot matter either
        std::vector<int> t0((size_t)N, 1);
        for (int i = 0; i < N; ++i)
            if (cond->known_types_host[i]) t0[i] = cond->types0_host[i];
        MI_TRY(upload(b, &b->cond_types0, (const int*)t0.data(), (size_t)N));
    }
    if (kx) MI_TRY(upload(b, &b->cond_frac0, cond->frac0_host, (size_t)N * 3));
    if (kl) MI_TRY(upload(b, &b->cond_lat0, cond->lat0_host, (size_t)B * 9));
    if (n > b->cond_table_cap) {
        MI_TRY(dev_alloc(b, &b->cond_table, (size_t)n * 3));
        b->cond_table_cap = n;
    }
    MI_HIP(hipMemcpy(b->cond_table, level_table_host, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
    b->cond_levels = n;
    b->cond_any = kt || kx || kl;
    b->cond_has_x = kx, b->cond_has_l = kl;
    b->cond_on = true;
    return MI_OK;
}

int mi_batch_set_likelihood_mask(mi_batch* b, const int* known_types, const int* known_coords, const int* known_lattice) {
    MI_NO_POOLED(b, "mi_batch_set_likelihood_mask");
    MI_CHECK(b, MI_EINVAL, "null handle");
    if (!known_types && !known_coords && !known_lattice) {
        b->lik_on = false;
        b->lik_h.clear();
        return MI_OK;
    }
    // every check first: a refused call leaves the handle as it was
    const int N = b->N, B = b->B;
    const int* part[3] = {known_types, known_coords, known_lattice};
    const int len[3] = {N, N, B};
    static const char* const name[3] = {"known_types", "known_coords", "known_lattice"};
    for (int k = 0; k < 3; ++k)
        for (int i = 0; part[k] && i < len[k]; ++i)
            MI_CHECK(part[k][i] == 0 || part[k][i] == 1, MI_EINVAL, "%s[%d] = %d: a likelihood mask holds 0 or 1", name[k], i, part[k][i]);
    std::vector<int> h((size_t)2 * N + B, 0);
    size_t off = 0;
    for (int k = 0; k < 3; off += (size_t)len[k], ++k)
        if (part[k]) std::copy(part[k], part[k] + len[k], h.begin() + off);
    b->lik_on = false;   // (a failed copy below leaves no half-written mask attached)
    MI_TRY(upload(b, &b->lik_kt, (const int*)h.data(), (size_t)N));
    MI_TRY(upload(b, &b->lik_kx, (const int*)h.data() + N, (size_t)N));
    MI_TRY(upload(b, &b->lik_kl, (const int*)h.data() + 2 * (size_t)N, (size_t)B));
    b->lik_h.swap(h);
    b->lik_on = true;
    return MI_OK;
}

int mi_batch_has_likelihood_mask(const mi_batch* b) {
    MI_CHECK(b, MI_EINVAL, "null handle");
    return b->lik_on ? 1 : 0;
}

int mi_condition_apply(mi_batch* b, int level, uint64_t seed, float* atom_types, float* frac, float* lattices, void* stream) {
    MI_NO_POOLED(b, "mi_condition_apply");
    MI_CHECK(b && atom_types && frac && lattices, MI_EINVAL, "null argument");
    return condition_impose(b, level, seed, atom_types, frac, lattices, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

}  // extern "C"
