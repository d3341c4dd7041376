// The elastic tensor and moduli of a learned energy (include/matinvent_hip_elastic.h).  Launches of this unit, no atomics, no
// scratch, no matrix pipe:
//   elastic_strain_kernel    one workgroup per strained copy: the source crystal's type rows (float4) and coordinates, the lattice L (I + eps);
//   elastic_collect_kernel   one thread per copy: its row sigma [6], V', flag of the workspace, float64, and asym from copy 12;
//   elastic_fit_kernel       one wave per crystal: C, S, the moduli, the eigenvalues and the counts, serially on its first lane with the
//                            work arrays in LDS.
// csrc/elastic_fit.h holds every formula, host and device.  mi_elastic_run_chunk enqueues strain, the ion relaxation (mi_relax_init and
// mi_relax_run at a fixed cell) when it is asked for, mi_scalar_input_grad and collect on one stream.

#include <climits>
#include <cmath>

#include "../../include/matinvent_hip_elastic.h"
#include "elastic_fit.h"
#include "energy_chunk.h"
#include "net.h"

namespace mi {

static_assert(ELASTIC_OK == MI_ELASTIC_OK && ELASTIC_BAD_INPUT == MI_ELASTIC_BAD_INPUT && ELASTIC_SINGULAR == MI_ELASTIC_SINGULAR, "status codes");
static_assert(ELASTIC_COPIES == MI_ELASTIC_COPIES && ELASTIC_ROW == MI_ELASTIC_ROW && RELAX_NI == MI_RELAX_NI, "sizes");
static_assert(RELAX_CONVERGED == MI_RELAX_CONVERGED && RELAX_FAILED == MI_RELAX_FAILED && RELAX_EXHAUSTED == MI_RELAX_EXHAUSTED, "relaxation codes");

constexpr int ELA_THREADS = 256;

struct ElasticChunk {
    mi_elastic_chunk_args a;
    const int* node_off;   // the chunk handle's
    int Bc;
    int relaxed;           // non-zero: a.istate is read
};

// the plan entry of copy k (energy_chunk.h): ELASTIC_COPIES copies of a crystal of any size
__device__ __forceinline__ bool ela_plan(const ElasticChunk& A, int k, int* src, int* c, int* n, int* s0, int* c0) {
    return chunk_plan_entry(A.a.plan_src, A.a.plan_copy, A.a.Bs, A.a.src_node_off, A.node_off, k, 0, ELASTIC_COPIES, INT_MAX, src, c, n, s0, c0);
}

__global__ __launch_bounds__(ELA_THREADS) void elastic_strain_kernel(ElasticChunk A) {
    const int k = blockIdx.x, tid = threadIdx.x;
    int src, c, n, s0, c0;
    if (!ela_plan(A, k, &src, &c, &n, &s0, &c0)) return;   // (uniform)
    chunk_copy_types(A.a.src_types, A.a.types, s0, c0, n, tid, ELA_THREADS);
    const float* xs = A.a.src_frac + (size_t)s0 * 3;
    float* xd = A.a.frac + (size_t)c0 * 3;
    for (int i = tid; i < n * 3; i += ELA_THREADS) xd[i] = xs[i];
    const float* lat = A.a.src_lat + (size_t)src * 9;
    double Li[9];
    const bool ok = vib_lattice(lat, A.a.det_min, Li);
    if (tid < 9) A.a.lat[(size_t)k * 9 + tid] = ok ? ela_strained(lat, A.a.h, c, tid / 3, tid % 3) : lat[tid];
}

__global__ __launch_bounds__(64) void elastic_collect_kernel(ElasticChunk A) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= A.Bc) return;
    int src, c, n, s0, c0;
    if (!ela_plan(A, k, &src, &c, &n, &s0, &c0)) return;
    const int ist = A.relaxed ? A.a.istate[(size_t)k * MI_RELAX_NI] : MI_RELAX_CONVERGED;
    double row[ELASTIC_ROW], asym;
    ela_collect_row(A.a.lat + (size_t)k * 9, A.a.g_lat + (size_t)k * 9, vib_scale(A.a.scale, A.a.per_atom, n), A.a.det_min, ist, row, &asym);
    double* dst = A.a.workspace + ((size_t)src * ELASTIC_COPIES + c) * ELASTIC_ROW;
#pragma unroll
    for (int i = 0; i < ELASTIC_ROW; ++i) dst[i] = row[i];
    if (c == ELASTIC_COPIES - 1) A.a.asym[src] = asym;
}

__global__ __launch_bounds__(64) void elastic_fit_kernel(mi_elastic_fit_args a) {
    __shared__ double work[ELASTIC_WORK];
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    ElasticFit o;
    o.C = a.C + (size_t)b * 36, o.S = a.S + (size_t)b * 36, o.stress0 = a.stress0 + (size_t)b * 6, o.moduli = a.moduli + (size_t)b * 15;
    o.evals = a.evals + (size_t)b * 6;
    ela_fit_crystal(a.workspace + (size_t)b * ELASTIC_COPIES * ELASTIC_ROW, a.h, work, &o);
    a.pressure[b] = o.pressure, a.asym_C[b] = o.asym_C, a.cond[b] = o.cond;
    a.n_negative[b] = o.n_negative, a.n_unrelaxed[b] = o.n_unrelaxed, a.status[b] = o.status;
    if (o.status == ELASTIC_BAD_INPUT) a.asym[b] = jac_nan();
}

static int ela_chunk_check(const char* what, const mi_batch* b, const mi_elastic_chunk_args* q) {
    return energy_chunk_check(what, "mi_elastic", b, q, q && q->g_lat && q->asym);
}

static int strain_launch(mi_batch* b, const mi_elastic_chunk_args* q, hipStream_t s) {
    ElasticChunk A{*q, b->node_off, b->B, 0};
    hipLaunchKernelGGL(elastic_strain_kernel, dim3(b->B), dim3(ELA_THREADS), 0, s, A);
    MI_KERNEL_CHECK();
    return MI_OK;
}

static int collect_launch(mi_batch* b, const mi_elastic_chunk_args* q, int relaxed, hipStream_t s) {
    ElasticChunk A{*q, b->node_off, b->B, relaxed};
    hipLaunchKernelGGL(elastic_collect_kernel, dim3((unsigned)cdiv(b->B, 64)), dim3(64), 0, s, A);
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_elastic_strain(mi_batch* b, const mi_elastic_chunk_args* args, void* stream) {
    MI_TRY(ela_chunk_check("mi_elastic_strain", b, args));
    if (b->B == 0 || b->N == 0) return MI_OK;
    return strain_launch(b, args, (hipStream_t)stream);
}

int mi_elastic_collect(mi_batch* b, const mi_elastic_chunk_args* args, void* stream) {
    MI_TRY(ela_chunk_check("mi_elastic_collect", b, args));
    if (b->B == 0 || b->N == 0) return MI_OK;
    return collect_launch(b, args, args->istate != nullptr, (hipStream_t)stream);
}

int mi_elastic_run_chunk(mi_net* net, mi_batch* b, const mi_elastic_chunk_args* args, const mi_relax_params* relax_params_host, int ion_steps,
                         const float* time_freqs, const float* W, const float* bias, int P, int p, float* d_out, float* out, float* vel_x,
                         float* fstate, void* stream) {
    const char* what = "mi_elastic_run_chunk";
    // mi_scalar_input_grad's refusals, by name, here (input_grad_refusals): the strain launch goes first, and nothing may be enqueued in
    // front of a refusal (its hidden_dim cap alone stays its own: a refusal there leaves a written chunk state and nothing else behind)
    MI_NO_LATENT(net, "mi_elastic_run_chunk");
    MI_NO_POOLED(b, "mi_elastic_run_chunk");
    MI_CHECK(net, MI_EINVAL, "%s: null network", what);
    MI_TRY(ela_chunk_check(what, b, args));
    MI_TRY(input_grad_refusals(what, net, b));
    MI_CHECK(P >= 1 && p >= 0 && p < P, MI_EINVAL, "%s: property p = %d of P = %d", what, p, P);
    MI_CHECK(ion_steps >= 0, MI_EINVAL, "%s: ion_steps = %d", what, ion_steps);
    mi_relax_params rp{};
    if (ion_steps > 0) {   // mi_relax_init's, mi_relax_step's and mi_relax_run's refusals
        MI_CHECK(relax_params_host, MI_EINVAL, "%s: null parameters", what);
        rp = *relax_params_host;
        rp.relax_cell = 0, rp.scale = (float)args->scale, rp.det_min = (float)args->det_min, rp.per_atom = args->per_atom ? 1 : 0;
        const float pos[] = {rp.dt, rp.dt_max, rp.maxstep, rp.f_inc, rp.f_dec, rp.a_start, rp.f_a, rp.fmax, rp.scale, rp.det_min};
        const char* names[] = {"dt", "dt_max", "maxstep", "f_inc", "f_dec", "a_start", "f_a", "fmax", "scale", "det_min"};
        for (int i = 0; i < 10; ++i)
            MI_CHECK(std::isfinite(pos[i]) && pos[i] > 0.f, MI_EINVAL, "%s: %s = %g: a relaxation parameter must be finite and positive", what, names[i], (double)pos[i]);
        MI_CHECK(std::isfinite(rp.cell_factor), MI_EINVAL, "%s: cell_factor is not finite", what);
        MI_CHECK(rp.n_min >= 0, MI_EINVAL, "%s: n_min = %d", what, rp.n_min);
        int largest = 0;
        for (int n : b->num_atoms_h) largest = std::max(largest, n);
        MI_CHECK(largest + 3 <= MI_RELAX_MAX_ROWS, MI_EINVAL, "%s: the handle's largest crystal has %d atoms (at most %d)", what, largest, MI_RELAX_MAX_ROWS - 3);
    }
    if (b->B == 0 || b->N == 0) return MI_OK;
    MI_CHECK(time_freqs && W && bias && d_out && out && args->g_frac, MI_EINVAL, "%s: null argument", what);
    MI_CHECK(ion_steps == 0 || (args->istate && vel_x && fstate), MI_EINVAL, "%s: null relaxation state", what);
    MI_TRY(strain_launch(b, args, (hipStream_t)stream));
    if (ion_steps > 0) {
        int* istate = const_cast<int*>(args->istate);
        MI_TRY(mi_relax_init(b, &rp, P, p, vel_x, nullptr, fstate, istate, d_out, stream));
        MI_TRY(mi_relax_run(net, b, &rp, args->types, args->frac, args->lat, time_freqs, W, bias, P, p, d_out, out, args->g_frac, args->g_lat, vel_x,
                            nullptr, fstate, istate, ion_steps, 1, stream));
    }
    MI_TRY(mi_scalar_input_grad(net, b, args->types, args->frac, args->lat, time_freqs, nullptr, 0, W, bias, P, d_out, out, nullptr, args->g_frac, args->g_lat, stream));
    return collect_launch(b, args, ion_steps > 0, (hipStream_t)stream);
}

int mi_elastic_fit(const mi_elastic_fit_args* args, void* stream) {
    MI_CHECK(args, MI_EINVAL, "mi_elastic_fit: null argument block");
    const mi_elastic_fit_args& a = *args;
    MI_CHECK(a.B >= 0, MI_EINVAL, "mi_elastic_fit: B = %d", a.B);
    MI_CHECK(pos_finite(a.h), MI_EINVAL, "mi_elastic_fit: h = %g: must be finite and positive", a.h);
    if (a.B == 0) return MI_OK;
    MI_CHECK(a.workspace && a.C && a.S && a.stress0 && a.pressure && a.asym && a.asym_C && a.moduli && a.evals && a.cond && a.n_negative && a.n_unrelaxed &&
                 a.status,
             MI_EINVAL, "mi_elastic_fit: null pointer");
    hipLaunchKernelGGL(elastic_fit_kernel, dim3(a.B), dim3(64), 0, (hipStream_t)stream, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // extern "C"
