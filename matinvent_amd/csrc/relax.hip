// Batched structure relaxation on a learned energy (include/matinvent_hip_relax.h): FIRE on the device, behind the property
// predictor's input gradient (input_grad.hip).  Launches of this unit, no atomics, no scratch:
//   relax_init_kernel     one thread per element: velocities 0, the per-crystal state, the constant seed d_out;
//   relax_step_kernel     one workgroup per crystal: the rows' forces and velocities in LDS, F.v / |v|^2 / |F|^2 / max |F row|^2 through ONE
//                         tree that is a function of the row count alone, the decision (uniform over the workgroup), |dr|^2 through the same
//                         tree, the clamp, the move (csrc/relax_fire.h holds every formula, host and device);
//   relax_finish_kernel   one thread per crystal: ACTIVE -> EXHAUSTED.
// mi_relax_run enqueues mi_scalar_input_grad + relax_step_kernel `steps` times on one stream: nothing waits for the host, a frozen crystal
// rides through every gradient evaluation and returns from the step kernel at its first instruction.

#include <cmath>

#include "../../include/matinvent_hip_relax.h"
#include "net.h"
#include "relax_fire.h"

namespace mi {

extern int g_edge_pairs;   // cspnet.hip (mi_set_edge_pairs)

static_assert(RELAX_ACTIVE == MI_RELAX_ACTIVE && RELAX_CONVERGED == MI_RELAX_CONVERGED && RELAX_FAILED == MI_RELAX_FAILED &&
                  RELAX_EXHAUSTED == MI_RELAX_EXHAUSTED && RELAX_NF == MI_RELAX_NF && RELAX_NI == MI_RELAX_NI,
              "status codes and state blocks");

__global__ __launch_bounds__(256) void relax_init_kernel(int N, int B, int P, int p, float dt, float a_start, float* __restrict__ vel_x,
                                                         float* __restrict__ vel_l, float* __restrict__ fs, int* __restrict__ is,
                                                         float* __restrict__ d_out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < (int64_t)N * 3) vel_x[idx] = 0.f;
    if (vel_l && idx < (int64_t)B * 9) vel_l[idx] = 0.f;
    if (idx < (int64_t)B * P) d_out[idx] = (int)(idx % P) == p ? 1.f : 0.f;
    if (idx < B) {
        float* f = fs + idx * RELAX_NF;
        f[RELAX_F_DT] = dt;
        f[RELAX_F_ALPHA] = a_start;
        f[RELAX_F_E_FIRST] = f[RELAX_F_E_LAST] = f[RELAX_F_FMAX] = f[RELAX_F_DR] = 0.f;
        int* i = is + idx * RELAX_NI;
        i[RELAX_I_STATUS] = RELAX_ACTIVE;
        i[RELAX_I_NPOS] = i[RELAX_I_STEPS] = 0;
    }
}

__global__ __launch_bounds__(256) void relax_finish_kernel(int B, int* __restrict__ is) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B && is[(size_t)b * RELAX_NI + RELAX_I_STATUS] == RELAX_ACTIVE) is[(size_t)b * RELAX_NI + RELAX_I_STATUS] = RELAX_EXHAUSTED;
}

struct RelaxStepArgs {
    const int* node_off;
    float *frac, *lat, *vel_x, *vel_l, *fs;
    int* is;
    const float *g_frac, *g_lat, *out;
    int P, p;
    RelaxParams prm;
};

// LDS: F [R][3] | v [R][3] | four sum arrays [R] each, R = the crystal's rows (the launch sizes it for the handle's largest crystal)
__global__ __launch_bounds__(256) void relax_step_kernel(RelaxStepArgs a) {
    extern __shared__ float lds[];
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    int* is = a.is + (size_t)b * RELAX_NI;
    if (is[RELAX_I_STATUS] != RELAX_ACTIVE) return;   // (uniform over the block; a frozen crystal keeps every bit)
    const RelaxParams& p = a.prm;
    const int n0 = a.node_off[b], n = a.node_off[b + 1] - n0;
    const int R = relax_rows(n, p.relax_cell);
    float *sF = lds, *sV = lds + 3 * R, *r0 = lds + 6 * R, *r1 = lds + 7 * R, *r2 = lds + 8 * R, *r3 = lds + 9 * R;
    float* lat = a.lat + (size_t)b * 9;
    float* x = a.frac + (size_t)n0 * 3;
    float* vx = a.vel_x + (size_t)n0 * 3;
    float* vl = p.relax_cell ? a.vel_l + (size_t)b * 9 : nullptr;
    const float* gl = a.g_lat + (size_t)b * 9;
    const float* gx = a.g_frac + (size_t)n0 * 3;
    const float out_p = a.out[(size_t)b * a.P + a.p];
    float L[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) L[q] = lat[q];
    int bad = 0;
    if (tid < 9 && !(guide_finite(gl[tid]) && guide_finite(lat[tid]))) bad = 1;
    if (tid == 0 && !guide_finite(out_p)) bad = 1;
    for (int i = tid; i < n * 3; i += T)
        if (!guide_finite(gx[i])) bad = 1;
    bad = __syncthreads_or(bad);
    const float det = relax_det3(L);
    if (bad || !(fabsf(det) >= p.det_min)) {   // (uniform)
        if (tid == 0) is[RELAX_I_STATUS] = RELAX_FAILED;
        return;
    }
    float Li[9];
    relax_inv3(L, det, Li);
    const float s = relax_force_scale(p, n), c = relax_cell_factor(p, n);
    for (int r = tid; r < R; r += T) {
        float F[3], v[3];
        if (r < n) relax_force_atom(gx + 3 * r, Li, s, F);
        else relax_force_cell(gl + 3 * (r - n), s, c, F);
        const float* vr = r < n ? vx + 3 * r : vl + 3 * (r - n);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v[k] = vr[k];
            sF[3 * r + k] = F[k];
            sV[3 * r + k] = v[k];
        }
        r0[r] = relax_dot3(F, v);
        r1[r] = relax_dot3(v, v);
        r2[r] = r3[r] = relax_dot3(F, F);
    }
    __syncthreads();
    const int half = relax_tree_half(R);
    for (int st = half; st > 0; st >>= 1) {
        for (int i = tid; i < st; i += T)
            if (i + st < R) {
                r0[i] += r0[i + st];
                r1[i] += r1[i + st];
                r2[i] += r2[i + st];
                r3[i] = r3[i + st] > r3[i] ? r3[i + st] : r3[i];
            }
        __syncthreads();
    }
    const float Pw = r0[0], vv = r1[0], ff = r2[0], fm = sqrtf(r3[0]);
    float* fs = a.fs + (size_t)b * RELAX_NF;
    const float dt0 = fs[RELAX_F_DT], alpha0 = fs[RELAX_F_ALPHA];
    const int npos0 = is[RELAX_I_NPOS], steps0 = is[RELAX_I_STEPS];
    if (tid == 0) {
        if (steps0 == 0) fs[RELAX_F_E_FIRST] = out_p;
        fs[RELAX_F_E_LAST] = out_p;
        fs[RELAX_F_FMAX] = fm;
    }
    if (fm < p.fmax) {   // (uniform) decided before any move
        if (tid == 0) is[RELAX_I_STATUS] = RELAX_CONVERGED;
        return;
    }
    const RelaxDecision d = relax_decide(Pw, vv, ff, dt0, alpha0, npos0, p);
    __syncthreads();   // (every thread has read the sums: r0 is reused)
    for (int r = tid; r < R; r += T) {
        float dr[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = relax_velocity(sV[3 * r + k], sF[3 * r + k], d);
            sV[3 * r + k] = v;
            dr[k] = d.dt * v;
            sF[3 * r + k] = dr[k];
        }
        r0[r] = relax_dot3(dr, dr);
    }
    __syncthreads();
    for (int st = half; st > 0; st >>= 1) {
        for (int i = tid; i < st; i += T)
            if (i + st < R) r0[i] += r0[i + st];
        __syncthreads();
    }
    const float nd = sqrtf(r0[0]);
    const float kc = relax_clamp(nd, p.maxstep);
    for (int r = tid; r < R; r += T) {
        const float dr[3] = {sF[3 * r] * kc, sF[3 * r + 1] * kc, sF[3 * r + 2] * kc};
        float* vr = r < n ? vx + 3 * r : vl + 3 * (r - n);
#pragma unroll
        for (int k = 0; k < 3; ++k) vr[k] = sV[3 * r + k];
        if (r < n) {
            float xr[3] = {x[3 * r], x[3 * r + 1], x[3 * r + 2]};
            relax_move_atom(xr, dr, Li);
#pragma unroll
            for (int k = 0; k < 3; ++k) x[3 * r + k] = xr[k];
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) lat[3 * (r - n) + k] = L[3 * (r - n) + k] + dr[k] / c;
        }
    }
    if (tid == 0) {
        fs[RELAX_F_DT] = d.dt;
        fs[RELAX_F_ALPHA] = d.alpha;
        fs[RELAX_F_DR] = nd;
        is[RELAX_I_NPOS] = d.npos;
        is[RELAX_I_STEPS] = steps0 + 1;
    }
}

static int relax_check(const char* what, const mi_batch* b, const mi_relax_params* q, int P, int p) {
    MI_CHECK(b, MI_EINVAL, "%s: null handle", what);
    MI_CHECK(q, MI_EINVAL, "%s: null parameters", what);
    const float pos[] = {q->dt, q->dt_max, q->maxstep, q->f_inc, q->f_dec, q->a_start, q->f_a, q->fmax, q->scale, q->det_min};
    const char* names[] = {"dt", "dt_max", "maxstep", "f_inc", "f_dec", "a_start", "f_a", "fmax", "scale", "det_min"};
    for (int i = 0; i < 10; ++i)
        MI_CHECK(std::isfinite(pos[i]) && pos[i] > 0.f, MI_EINVAL, "%s: %s = %g: a relaxation parameter must be finite and positive", what, names[i], (double)pos[i]);
    MI_CHECK(std::isfinite(q->cell_factor), MI_EINVAL, "%s: cell_factor is not finite", what);
    MI_CHECK(q->n_min >= 0, MI_EINVAL, "%s: n_min = %d", what, q->n_min);
    MI_CHECK(P >= 1 && p >= 0 && p < P, MI_EINVAL, "%s: property p = %d of P = %d", what, p, P);
    return MI_OK;
}

static RelaxParams relax_params(const mi_relax_params* q) {
    RelaxParams r;
    r.dt = q->dt, r.dt_max = q->dt_max, r.maxstep = q->maxstep, r.f_inc = q->f_inc, r.f_dec = q->f_dec, r.a_start = q->a_start, r.f_a = q->f_a;
    r.fmax = q->fmax, r.scale = q->scale, r.cell_factor = q->cell_factor, r.det_min = q->det_min;
    r.n_min = q->n_min, r.relax_cell = q->relax_cell ? 1 : 0, r.per_atom = q->per_atom ? 1 : 0;
    return r;
}

static int relax_largest(const mi_batch* b) {
    int m = 0;
    for (int n : b->num_atoms_h) m = std::max(m, n);
    return m;
}

static int relax_step_launch(const char* what, mi_batch* b, const mi_relax_params* q, int P, int p, float* frac, float* lattices, float* vel_x,
                             float* vel_l, float* fstate, int* istate, const float* g_frac, const float* g_lat, const float* out, hipStream_t s) {
    const int rows = relax_largest(b) + 3;
    MI_CHECK(rows <= MI_RELAX_MAX_ROWS, MI_EINVAL, "%s: the handle's largest crystal has %d atoms (at most %d)", what, rows - 3, MI_RELAX_MAX_ROWS - 3);
    int T = 64;
    while (T < rows && T < 256) T <<= 1;
    RelaxStepArgs a{b->node_off, frac, lattices, vel_x, vel_l, fstate, istate, g_frac, g_lat, out, P, p, relax_params(q)};
    hipLaunchKernelGGL(relax_step_kernel, dim3(b->B), dim3(T), (size_t)rows * 10 * sizeof(float), s, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_relax_init(mi_batch* b, const mi_relax_params* params_host, int P, int p, float* vel_x, float* vel_l, float* fstate, int* istate,
                  float* d_out, void* stream) {
    const char* what = "mi_relax_init";
    MI_TRY(relax_check(what, b, params_host, P, p));
    MI_POOL_STREAM(b, stream, "mi_relax_init");
    if (b->B == 0) return MI_OK;
    MI_CHECK(vel_x && fstate && istate && d_out && (vel_l || !params_host->relax_cell), MI_EINVAL, "%s: null argument", what);
    const int64_t m = std::max<int64_t>(std::max<int64_t>((int64_t)b->N * 3, (int64_t)b->B * 9), (int64_t)b->B * P);
    hipLaunchKernelGGL(relax_init_kernel, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, (hipStream_t)stream, b->N, b->B, P, p, params_host->dt,
                       params_host->a_start, vel_x, vel_l, fstate, istate, d_out);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int mi_relax_step(mi_batch* b, const mi_relax_params* params_host, int P, int p, float* frac, float* lattices, float* vel_x, float* vel_l,
                  float* fstate, int* istate, const float* g_frac, const float* g_lat, const float* out, void* stream) {
    const char* what = "mi_relax_step";
    MI_TRY(relax_check(what, b, params_host, P, p));
    MI_POOL_STREAM(b, stream, "mi_relax_step");
    if (b->B == 0) return MI_OK;
    MI_CHECK(frac && lattices && vel_x && fstate && istate && g_frac && g_lat && out && (vel_l || !params_host->relax_cell), MI_EINVAL,
             "%s: null argument", what);
    return relax_step_launch(what, b, params_host, P, p, frac, lattices, vel_x, vel_l, fstate, istate, g_frac, g_lat, out, (hipStream_t)stream);
}

int mi_relax_run(mi_net* net, mi_batch* b, const mi_relax_params* params_host, const float* atom_types, float* frac, float* lattices,
                 const float* time_freqs, const float* W, const float* bias, int P, int p, const float* d_out, float* out, float* g_frac,
                 float* g_lat, float* vel_x, float* vel_l, float* fstate, int* istate, int steps, int finish, void* stream) {
    const char* what = "mi_relax_run";
    // mi_scalar_input_grad's refusals that need no call of it (the others are its own, at the first iteration, before it enqueues anything,
    // under its own name: input_grad_refusals (net.h) would rename them, so this prefix of its list stays written out)
    MI_NO_LATENT(net, "mi_relax_run");
    MI_NO_POOLED(b, "mi_relax_run");
    MI_CHECK(net, MI_EINVAL, "%s: null network", what);
    MI_TRY(relax_check(what, b, params_host, P, p));
    MI_CHECK(!b->knn, MI_EINVAL, "%s: a knn-style handle (the input gradient runs in the fully connected pair mode only)", what);
    MI_CHECK(g_edge_pairs && net->H % 4 == 0, MI_EINVAL, "%s: pair mode is off or hidden_dim %% 4 != 0 (the input gradient runs in pair mode only)", what);
    MI_CHECK(b->tape.wslots == 0, MI_EINVAL, "%s: the handle has an open weight-gradient window (mi_batch_set_wgrad_window(.., 0) first)", what);
    MI_CHECK(steps >= 0, MI_EINVAL, "%s: steps = %d", what, steps);
    MI_CHECK(relax_largest(b) + 3 <= MI_RELAX_MAX_ROWS, MI_EINVAL, "%s: the handle's largest crystal has %d atoms (at most %d)", what, relax_largest(b),
             MI_RELAX_MAX_ROWS - 3);
    if (b->B == 0 || b->N == 0 || steps == 0) return MI_OK;
    MI_CHECK(atom_types && frac && lattices && d_out && out && g_frac && g_lat && vel_x && fstate && istate && (vel_l || !params_host->relax_cell),
             MI_EINVAL, "%s: null argument", what);
    for (int k = 0; k < steps; ++k) {
        MI_TRY(mi_scalar_input_grad(net, b, atom_types, frac, lattices, time_freqs, nullptr, 0, W, bias, P, d_out, out, nullptr, g_frac, g_lat, stream));
        MI_TRY(relax_step_launch(what, b, params_host, P, p, frac, lattices, vel_x, vel_l, fstate, istate, g_frac, g_lat, out, (hipStream_t)stream));
    }
    if (finish) {
        hipLaunchKernelGGL(relax_finish_kernel, dim3((unsigned)cdiv(b->B, 256)), dim3(256), 0, (hipStream_t)stream, b->B, istate);
        MI_KERNEL_CHECK();
    }
    return MI_OK;
}

}  // extern "C"
