// Gamma-point vibrations of a learned energy (include/matinvent_hip_vib.h).  Launches of this unit, no atomics, no scratch, no
// matrix pipe:
//   vib_displace_kernel   one workgroup per displaced copy: the source crystal's type rows (float4), coordinates and lattice, one atom moved;
//   vib_collect_kernel    one wave per displaced copy: its row of Cartesian gradients Gc in the workspace, float64;
//   vib_dynmat_kernel     one workgroup per crystal: the central-difference Hessian, asym, the symmetrisation, the acoustic sum rule, the mass
//                         weighting and the three Householder reflections in the workspace's W, the vibrational block R;
//   sym_eig_kernel        one workgroup per matrix: cyclic Jacobi in the round-robin ordering, the matrix in LDS when it fits and in the
//                         workspace otherwise (the same element formulas on either pointer: the same bits), the ranked diagonal;
//   vib_thermo_kernel     one wave per crystal: frequencies, counts, c_v at up to 8 temperatures, the zero-point energy.
// csrc/vib_dynmat.h and csrc/sym_jacobi.h hold every formula, host and device.  mi_vib_run_chunk enqueues displace, mi_scalar_input_grad and
// collect on one stream.

#include <cmath>
#include <mutex>

#include "../../include/matinvent_hip_vib.h"
#include "energy_chunk.h"
#include "net.h"
#include "vib_dynmat.h"

namespace mi {

static_assert(VIB_OK == MI_VIB_OK && VIB_NO_CONVERGENCE == MI_VIB_NO_CONVERGENCE && VIB_BAD_INPUT == MI_VIB_BAD_INPUT && EIG_OK == MI_VIB_OK &&
                  EIG_NO_CONVERGENCE == MI_VIB_NO_CONVERGENCE && EIG_BAD_INPUT == MI_VIB_BAD_INPUT,
              "status codes");
static_assert(VIB_MAX_ATOMS == MI_VIB_MAX_ATOMS && VIB_MAX_TEMPS == MI_VIB_MAX_TEMPS && EIG_MAX_SWEEPS == MI_EIG_MAX_SWEEPS &&
                  EIG_LDS_MAX_M == MI_EIG_LDS_MAX_M && EIG_MAX_M == MI_EIG_MAX_M && 3 * VIB_MAX_ATOMS <= EIG_MAX_M,
              "sizes");

constexpr int VIB_THREADS = 256;

struct VibChunk {
    mi_vib_chunk_args a;
    const int* node_off;   // the chunk handle's
    int Bc;
};

// the plan entry of copy k (energy_chunk.h): 6 n copies of a crystal of n <= VIB_MAX_ATOMS atoms
__device__ __forceinline__ bool vib_plan(const VibChunk& A, int k, int* src, int* c, int* n, int* s0, int* c0) {
    return chunk_plan_entry(A.a.plan_src, A.a.plan_copy, A.a.Bs, A.a.src_node_off, A.node_off, k, 6, 0, VIB_MAX_ATOMS, src, c, n, s0, c0);
}

__global__ __launch_bounds__(VIB_THREADS) void vib_displace_kernel(VibChunk A) {
    const int k = blockIdx.x, tid = threadIdx.x;
    int src, c, n, s0, c0;
    if (!vib_plan(A, k, &src, &c, &n, &s0, &c0)) return;
    chunk_copy_types(A.a.src_types, A.a.types, s0, c0, n, tid, VIB_THREADS);
    const float* lat = A.a.src_lat + (size_t)src * 9;
    if (tid < 9) A.a.lat[(size_t)k * 9 + tid] = lat[tid];
    double Li[9];
    const bool ok = vib_lattice(lat, A.a.det_min, Li);
    const int atom = c / 6, d = (c % 6) / 2, s = c & 1;
    const float* xs = A.a.src_frac + (size_t)s0 * 3;
    float* xd = A.a.frac + (size_t)c0 * 3;
    for (int i = tid; i < n * 3; i += VIB_THREADS) xd[i] = (ok && i / 3 == atom) ? vib_displaced(xs[i], A.a.h, d, s, i % 3, Li) : xs[i];
}

__global__ __launch_bounds__(64) void vib_collect_kernel(VibChunk A) {
    const int k = blockIdx.x, tid = threadIdx.x;
    int src, c, n, s0, c0;
    if (!vib_plan(A, k, &src, &c, &n, &s0, &c0)) return;
    double Li[9];
    const bool ok = vib_lattice(A.a.lat + (size_t)k * 9, A.a.det_min, Li);
    const double s = vib_scale(A.a.scale, A.a.per_atom, n);
    const float* g = A.a.g_frac + (size_t)c0 * 3;
    double* row = A.a.workspace + A.a.ws_off[src] + (size_t)c * 3 * n;
    for (int i = tid; i < n * 3; i += 64) row[i] = ok ? vib_cart_grad(g + 3 * (i / 3), Li, s, i % 3) : jac_nan();
}

__global__ __launch_bounds__(VIB_THREADS) void vib_dynmat_kernel(mi_vib_dynmat_args a) {
    __shared__ double sv[3 * 3 * VIB_MAX_ATOMS];   // the three Householder vectors
    __shared__ double sw[3 * 3 * VIB_MAX_ATOMS];   // their work columns U, then w = D v in the first third
    __shared__ double red[VIB_THREADS / 64];
    __shared__ double sK;
    const int b = blockIdx.x, tid = threadIdx.x, T = VIB_THREADS;
    const int n0 = a.node_off[b], n = a.node_off[b + 1] - n0;
    if (n < 1 || n > a.max_atoms) {   // (uniform) nothing is addressed with such a count
        if (tid == 0) a.status[b] = VIB_BAD_INPUT, a.asym[b] = jac_nan();
        return;
    }
    const int N3 = 3 * n, M = vib_modes(n);
    const size_t NN = (size_t)N3 * N3;
    const double* mass = a.mass + n0;
    const double* Gc = a.workspace + a.ws_off[b];
    double* W = a.workspace + a.ws_off[b] + 18 * (size_t)n * n;
    double* R = a.workspace + a.ws_off[b] + 27 * (size_t)n * n;
    int bad = 0;
    for (size_t i = tid; i < 2 * NN; i += T) bad |= !jac_finite(Gc[i]);
    for (int j = tid; j < n; j += T) bad |= !(jac_finite(mass[j]) && mass[j] > 0.0);
    bad = __syncthreads_or(bad);
    if (bad) {   // (uniform)
        for (size_t i = tid; i < (size_t)M * M; i += T) R[i] = jac_nan();
        if (tid == 0) a.status[b] = VIB_BAD_INPUT, a.asym[b] = jac_nan();
        return;
    }
    const double two_h = 2.0 * a.h;
    for (size_t i = tid; i < NN; i += T) {
        const size_t r = i / N3, c = i % N3;
        W[i] = vib_hessian(Gc[(2 * r) * N3 + c], Gc[(2 * r + 1) * N3 + c], two_h);
    }
    __syncthreads();
    double mh = 0.0, md = 0.0;
    for (size_t i = tid; i < NN; i += T) {
        const size_t r = i / N3, c = i % N3;
        const double x = fabs(W[i]), y = fabs(W[i] - W[c * N3 + r]);
        mh = x > mh ? x : mh, md = y > md ? y : md;
    }
    mh = block_max_f64<VIB_THREADS>(mh, red, tid);
    md = block_max_f64<VIB_THREADS>(md, red, tid);   // (its first barrier also closes the reads of W above)
    if (tid == 0) a.asym[b] = mh > 0.0 ? md / mh : 0.0, a.status[b] = VIB_OK;
    for (size_t i = tid; i < NN; i += T) {   // the pair (r, c), r < c, is written by the thread of its upper element
        const size_t r = i / N3, c = i % N3;
        if (r < c) W[i] = W[c * N3 + r] = vib_mean(W[i], W[c * N3 + r]);
    }
    __syncthreads();
    for (int i = tid; i < 9 * n; i += T) {   // reads the blocks j != i only, writes block (i, i)
        const int at = i / 9, d = (i % 9) / 3, e = i % 3;
        W[(size_t)(3 * at + d) * N3 + 3 * at + e] = vib_asr(W, N3, n, at, d, e);
    }
    __syncthreads();
    for (int i = tid; i < 9 * n; i += T) {
        const int at = i / 9, d = (i % 9) / 3, e = i % 3;
        if (d < e) {
            double* p = W + (size_t)(3 * at + d) * N3 + 3 * at + e;
            double* q = W + (size_t)(3 * at + e) * N3 + 3 * at + d;
            *p = *q = vib_mean(*p, *q);
        }
    }
    __syncthreads();
    for (size_t i = tid; i < NN; i += T) W[i] = vib_mass_weight(W[i], mass[(i / N3) / 3], mass[(i % N3) / 3]);
    if (M == 0) return;   // (uniform) one atom: no modes
    if (tid == 0) vib_householder(mass, n, sv, sw);
    __syncthreads();
    for (int k = 0; k < 3; ++k) {
        const double* vk = sv + k * N3;
        for (int r = tid; r < N3; r += T) sw[r] = vib_row_dot(W, N3, r, vk);
        __syncthreads();
        if (tid == 0) sK = vib_dot(vk, sw, N3);
        __syncthreads();
        const double K = sK;
        for (size_t i = tid; i < NN; i += T) {
            const size_t r = i / N3, c = i % N3;
            W[i] = vib_reflect(W[i], vk[r], vk[c], sw[r], sw[c], K);
        }
        __syncthreads();
    }
    for (size_t i = tid; i < (size_t)M * M; i += T) {
        const size_t x = i / M, y = i % M;
        R[i] = vib_mean(W[(3 + x) * N3 + 3 + y], W[(3 + y) * N3 + 3 + x]);
    }
}

// LDS: rc | rs | rpp | rqq [np] doubles, rp | rq | rrot [np] ints (np: the pairs of the largest matrix), then the matrix when it sits there
__global__ __launch_bounds__(VIB_THREADS) void sym_eig_kernel(mi_sym_eig_args a, int np_max, int lds_m) {
    extern __shared__ double eig_lds[];
    const int b = blockIdx.x, tid = threadIdx.x, T = VIB_THREADS;
    const int M = a.sizes[b];
    if (M < 0 || M > a.max_size) {   // (uniform)
        if (tid == 0) a.status[b] = EIG_BAD_INPUT, a.sweeps[b] = 0;
        return;
    }
    double *rc = eig_lds, *rs = rc + np_max, *rpp = rs + np_max, *rqq = rpp + np_max;
    int *rp = reinterpret_cast<int*>(rqq + np_max), *rq = rp + np_max, *rrot = rq + np_max;
    const double* src = a.mats + a.mat_off[b];
    double* ev = a.evals + a.ev_off[b];
    const size_t MM = (size_t)M * M;
    int bad = 0;
    for (size_t i = tid; i < MM; i += T) bad |= !jac_finite(src[i]);
    bad = __syncthreads_or(bad);
    if (bad) {   // (uniform)
        for (int i = tid; i < M; i += T) ev[i] = jac_nan();
        if (tid == 0) a.status[b] = EIG_BAD_INPUT, a.sweeps[b] = 0;
        return;
    }
    // the rotated copy: LDS behind the pair arrays (8-byte aligned: 4 np doubles + 3 np ints, np_max even or the ints padded by the launcher)
    double* A = (M <= lds_m) ? reinterpret_cast<double*>(rrot + np_max + (np_max & 1)) : a.work + (a.work_off ? a.work_off[b] : a.mat_off[b]);
    for (size_t i = tid; i < MM; i += T) A[i] = src[i];
    __syncthreads();
    const int Me = jac_even(M), np = Me / 2;
    int done = 0, status = EIG_NO_CONVERGENCE;
    for (int sw = 0; sw < EIG_MAX_SWEEPS; ++sw) {
        int any_sweep = 0;
        for (int r = 0; r < Me - 1; ++r) {
            int rot = 0;
            for (int k = tid; k < np; k += T) {
                int p, q;
                jac_pair(Me, r, k, &p, &q);
                rp[k] = p, rq[k] = q, rrot[k] = 0;
                if (q < M) {
                    const JacRot R = jac_rotation(A[(size_t)p * M + p], A[(size_t)q * M + q], A[(size_t)p * M + q]);
                    rc[k] = R.c, rs[k] = R.s, rpp[k] = R.pp, rqq[k] = R.qq, rrot[k] = R.rot;
                    rot |= R.rot;
                }
            }
            rot = __syncthreads_or(rot);
            if (!rot) continue;   // (uniform; the next round's writes of the pair arrays follow every read of this one: none was made)
            any_sweep = 1;
            for (int i = tid; i < M * np; i += T) {   // columns: (row i / np, pair i % np)
                const int row = i / np, k = i % np;
                if (!rrot[k]) continue;
                double* x = A + (size_t)row * M + rp[k];
                double* y = A + (size_t)row * M + rq[k];
                const double xv = *x, yv = *y;
                *x = jac_first(rc[k], rs[k], xv, yv);
                *y = jac_second(rc[k], rs[k], xv, yv);
            }
            __syncthreads();
            for (int i = tid; i < np * M; i += T) {   // rows: (pair i / M, column i % M)
                const int k = i / M, j = i % M;
                if (!rrot[k]) continue;
                const int p = rp[k], q = rq[k];
                double* x = A + (size_t)p * M + j;
                double* y = A + (size_t)q * M + j;
                const double xv = *x, yv = *y;
                *x = j == p ? rpp[k] : (j == q ? 0.0 : jac_first(rc[k], rs[k], xv, yv));
                *y = j == q ? rqq[k] : (j == p ? 0.0 : jac_second(rc[k], rs[k], xv, yv));
            }
            __syncthreads();
        }
        if (!any_sweep) {
            status = EIG_OK;
            break;
        }
        ++done;
    }
    for (int i = tid; i < M; i += T) ev[jac_rank(A, M, M, i)] = A[(size_t)i * M + i];
    if (tid == 0) a.status[b] = status, a.sweeps[b] = done;
}

__global__ __launch_bounds__(64) void vib_thermo_kernel(mi_vib_thermo_args a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int M = a.sizes[b], dst = a.dyn_status ? a.dyn_status[b] : VIB_OK, st = dst != VIB_OK ? dst : a.eig_status[b];
    const double* lam = a.evals + a.ev_off[b];
    double* nu = a.freqs + a.ev_off[b];
    const bool ok = st == VIB_OK && M >= 0;
    if (M > 0)
        for (int k = tid; k < M; k += 64) nu[k] = ok ? vib_frequency(lam[k]) : jac_nan();
    if (tid < a.K) a.c_v[(size_t)b * a.K + tid] = ok ? vib_cv(lam, M, a.nu_cut, a.temps[tid]) : jac_nan();
    if (tid == VIB_MAX_TEMPS) {
        int ni = -1, nz = -1;
        const double z = ok ? vib_zpe(lam, M, a.nu_cut, &ni, &nz) : jac_nan();
        a.zpe[b] = z, a.n_imag[b] = ni, a.n_zero[b] = nz, a.status[b] = ok ? VIB_OK : (st == VIB_OK ? VIB_BAD_INPUT : st);
    }
}

static int chunk_check(const char* what, const mi_batch* b, const mi_vib_chunk_args* q) {
    return energy_chunk_check(what, "mi_vib", b, q, q && q->g_frac && q->ws_off);
}

static int displace_launch(mi_batch* b, const mi_vib_chunk_args* q, hipStream_t s) {
    VibChunk A{*q, b->node_off, b->B};
    hipLaunchKernelGGL(vib_displace_kernel, dim3(b->B), dim3(VIB_THREADS), 0, s, A);
    MI_KERNEL_CHECK();
    return MI_OK;
}

static int collect_launch(mi_batch* b, const mi_vib_chunk_args* q, hipStream_t s) {
    VibChunk A{*q, b->node_off, b->B};
    hipLaunchKernelGGL(vib_collect_kernel, dim3(b->B), dim3(64), 0, s, A);
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int64_t mi_vib_workspace(const int* num_atoms_host, int B, int64_t* offsets_host) {
    MI_CHECK(B >= 0 && (num_atoms_host || B == 0), MI_EINVAL, "mi_vib_workspace: B = %d or a null list", B);
    int64_t o = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = num_atoms_host[b], M = 3 * n - 3;
        MI_CHECK(n >= 1 && n <= MI_VIB_MAX_ATOMS, MI_EINVAL, "mi_vib_workspace: crystal %d has %d atoms (1 .. %d)", b, (int)n, MI_VIB_MAX_ATOMS);
        if (offsets_host) offsets_host[b] = o;
        o += 27 * n * n + 2 * M * M;
    }
    if (offsets_host) offsets_host[B] = o;
    return o * (int64_t)sizeof(double);
}

int mi_vib_displace(mi_batch* b, const mi_vib_chunk_args* args, void* stream) {
    MI_TRY(chunk_check("mi_vib_displace", b, args));
    if (b->B == 0 || b->N == 0) return MI_OK;
    return displace_launch(b, args, (hipStream_t)stream);
}

int mi_vib_collect(mi_batch* b, const mi_vib_chunk_args* args, void* stream) {
    MI_TRY(chunk_check("mi_vib_collect", b, args));
    if (b->B == 0 || b->N == 0) return MI_OK;
    return collect_launch(b, args, (hipStream_t)stream);
}

int mi_vib_run_chunk(mi_net* net, mi_batch* b, const mi_vib_chunk_args* args, const float* time_freqs, const float* W, const float* bias, int P,
                     const float* d_out, float* out, float* g_lat, void* stream) {
    const char* what = "mi_vib_run_chunk";
    // mi_scalar_input_grad's refusals, by name, here (input_grad_refusals): the displace launch goes first, and nothing may be enqueued in
    // front of a refusal (its hidden_dim cap alone stays its own: a refusal there leaves a written chunk state and nothing else behind)
    MI_NO_LATENT(net, "mi_vib_run_chunk");
    MI_NO_POOLED(b, "mi_vib_run_chunk");
    MI_CHECK(net, MI_EINVAL, "%s: null network", what);
    MI_TRY(chunk_check(what, b, args));
    MI_TRY(input_grad_refusals(what, net, b));
    MI_CHECK(P >= 1, MI_EINVAL, "%s: P = %d", what, P);
    if (b->B == 0 || b->N == 0) return MI_OK;
    MI_CHECK(time_freqs && W && bias && d_out && out && g_lat, MI_EINVAL, "%s: null argument", what);
    MI_TRY(displace_launch(b, args, (hipStream_t)stream));
    MI_TRY(mi_scalar_input_grad(net, b, args->types, args->frac, args->lat, time_freqs, nullptr, 0, W, bias, P, d_out, out, nullptr, args->g_frac, g_lat, stream));
    return collect_launch(b, args, (hipStream_t)stream);
}

int mi_vib_dynmat(const mi_vib_dynmat_args* args, void* stream) {
    MI_CHECK(args, MI_EINVAL, "mi_vib_dynmat: null argument block");
    const mi_vib_dynmat_args& a = *args;
    MI_CHECK(a.B >= 0, MI_EINVAL, "mi_vib_dynmat: B = %d", a.B);
    MI_CHECK(pos_finite(a.h), MI_EINVAL, "mi_vib_dynmat: h = %g: must be finite and positive", a.h);
    MI_CHECK(a.max_atoms >= 1 && a.max_atoms <= MI_VIB_MAX_ATOMS, MI_EINVAL, "mi_vib_dynmat: max_atoms = %d outside 1..%d", a.max_atoms, MI_VIB_MAX_ATOMS);
    if (a.B == 0) return MI_OK;
    MI_CHECK(a.workspace && a.ws_off && a.node_off && a.mass && a.asym && a.status, MI_EINVAL, "mi_vib_dynmat: null pointer");
    hipLaunchKernelGGL(vib_dynmat_kernel, dim3(a.B), dim3(VIB_THREADS), 0, (hipStream_t)stream, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int mi_sym_eigvals(const mi_sym_eig_args* args, void* stream) {
    MI_CHECK(args, MI_EINVAL, "mi_sym_eigvals: null argument block");
    const mi_sym_eig_args& a = *args;
    MI_CHECK(a.B >= 0, MI_EINVAL, "mi_sym_eigvals: B = %d", a.B);
    MI_CHECK(a.max_size >= 0 && a.max_size <= MI_EIG_MAX_M, MI_EINVAL, "mi_sym_eigvals: max_size = %d outside 0..%d", a.max_size, MI_EIG_MAX_M);
    if (a.B == 0) return MI_OK;
    MI_CHECK(a.mats && a.mat_off && a.sizes && a.evals && a.ev_off && a.sweeps && a.status, MI_EINVAL, "mi_sym_eigvals: null pointer");
    const int lds_m = a.no_lds ? -1 : std::min(a.max_size, (int)MI_EIG_LDS_MAX_M);   // the largest order that is rotated in LDS
    MI_CHECK(a.work || (!a.no_lds && a.max_size <= MI_EIG_LDS_MAX_M), MI_EINVAL, "mi_sym_eigvals: no work array, but max_size = %d (no_lds = %d) needs one",
             a.max_size, a.no_lds);
    const int np_max = std::max(1, (a.max_size + 1) / 2);
    const size_t pair_bytes = (size_t)np_max * 4 * sizeof(double) + (size_t)(np_max + (np_max & 1)) * 3 * sizeof(int) + 8;
    const size_t lds = pair_bytes + (lds_m > 0 ? (size_t)lds_m * lds_m * sizeof(double) : 0);
    static std::once_flag once;
    static hipError_t attr_err = hipSuccess;
    std::call_once(once, [] {
        attr_err = hipFuncSetAttribute((const void*)sym_eig_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       MI_EIG_LDS_MAX_M * MI_EIG_LDS_MAX_M * (int)sizeof(double) + 20 * 1024);   // (the pair arrays of order 768: 17 KiB)
    });
    MI_HIP(attr_err);
    hipLaunchKernelGGL(sym_eig_kernel, dim3(a.B), dim3(VIB_THREADS), lds, (hipStream_t)stream, a, np_max, lds_m);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int mi_vib_thermo(const mi_vib_thermo_args* args, void* stream) {
    MI_CHECK(args, MI_EINVAL, "mi_vib_thermo: null argument block");
    const mi_vib_thermo_args& a = *args;
    MI_CHECK(a.B >= 0, MI_EINVAL, "mi_vib_thermo: B = %d", a.B);
    MI_CHECK(a.K >= 1 && a.K <= MI_VIB_MAX_TEMPS, MI_EINVAL, "mi_vib_thermo: K = %d outside 1..%d", a.K, MI_VIB_MAX_TEMPS);
    for (int k = 0; k < a.K; ++k) MI_CHECK(pos_finite(a.temps[k]), MI_EINVAL, "mi_vib_thermo: temperature %d = %g: must be finite and positive", k, a.temps[k]);
    MI_CHECK(std::isfinite(a.nu_cut) && a.nu_cut >= 0.0, MI_EINVAL, "mi_vib_thermo: nu_cut = %g", a.nu_cut);
    if (a.B == 0) return MI_OK;
    MI_CHECK(a.evals && a.ev_off && a.sizes && a.eig_status && a.freqs && a.c_v && a.zpe && a.n_imag && a.n_zero && a.status, MI_EINVAL, "mi_vib_thermo: null pointer");
    hipLaunchKernelGGL(vib_thermo_kernel, dim3(a.B), dim3(64), 0, (hipStream_t)stream, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // extern "C"
