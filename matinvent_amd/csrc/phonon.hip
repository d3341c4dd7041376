// Phonons on a q-mesh from home-cell displacements in a supercell (include/matinvent_hip_phonon.h).  Launches of this unit, no
// atomics, no scratch, no matrix pipe, no transcendental function:
//   phonon_fc_kernel       one workgroup per supercell: the central-difference force constants Phi of the home cell's atoms, asym, the index
//                          symmetry, the acoustic sum rule and the shortest-image masks, in the workspace;
//   phonon_dynmat_kernel   one workgroup per (crystal, q) item, a thread per matrix element: D(q) from Phi, the masks and the host's phase
//                          table, herm, the Hermitian part, and its real symmetric embedding of order 6 n where mi_sym_eigvals reads it;
//   phonon_thermo_kernel   one wave per crystal: the eigenvalue pairs' means, pair_gap, frequencies, the weighted counts, c_v at up to 8
//                          temperatures, the zero-point energy, the lowest frequency and its q.
// csrc/phonon_fc.h holds every formula, host and device.  The gradients are mi_vib_run_chunk's and the eigenvalues mi_sym_eigvals' (vib.hip),
// called by the host as they stand.

#include <cmath>

#include "../../include/matinvent_hip_phonon.h"
#include "energy_chunk.h"
#include "phonon_fc.h"

namespace mi {

static_assert(PH_MAX_PRIM == MI_PHONON_MAX_PRIM && PH_IMAGES == MI_PHONON_IMAGES && 6 * PH_MAX_PRIM <= MI_EIG_MAX_M, "sizes");
static_assert(VIB_OK == MI_VIB_OK && VIB_BAD_INPUT == MI_VIB_BAD_INPUT && VIB_NO_CONVERGENCE == MI_VIB_NO_CONVERGENCE, "status codes");

constexpr int PH_THREADS = 256;

// the primitive cell's atom count of a supercell of Ns atoms; 0: not admissible
__device__ __forceinline__ int ph_prim_atoms(int Ns, int N, int max_atoms) {
    if (Ns < 1 || Ns > max_atoms || N < 1 || Ns % N != 0 || Ns / N > PH_MAX_PRIM) return 0;
    return Ns / N;
}

__global__ __launch_bounds__(PH_THREADS) void phonon_fc_kernel(mi_phonon_fc_args a) {
    __shared__ double red[PH_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, T = PH_THREADS;
    const int reps[3] = {a.reps[0], a.reps[1], a.reps[2]};
    const int n0 = a.node_off[b], Ns = a.node_off[b + 1] - n0;
    const int n = ph_prim_atoms(Ns, ph_images(reps), a.max_atoms);
    if (n == 0) {   // (uniform) nothing is addressed with such a count
        if (tid == 0) a.status[b] = VIB_BAD_INPUT, a.asym[b] = jac_nan();
        return;
    }
    const size_t W = (size_t)3 * Ns, total = (size_t)3 * n * W;
    const double* mass = a.mass + n0;
    const float* frac = a.frac + (size_t)3 * n0;
    const double* Gc = a.workspace + a.ws_off[b];
    double* Phi = a.workspace + a.ws_off[b] + 2 * total;
    int* masks = reinterpret_cast<int*>(a.workspace + a.ws_off[b] + 3 * total);
    double L[9];
    int bad = !ph_lattice(a.lat + (size_t)9 * b, a.det_min, L);
    for (size_t i = tid; i < 2 * total; i += T) bad |= !jac_finite(Gc[i]);
    for (int j = tid; j < n; j += T) bad |= !(jac_finite(mass[j]) && mass[j] > 0.0);
    bad = __syncthreads_or(bad);
    if (bad) {   // (uniform)
        for (size_t i = tid; i < total; i += T) Phi[i] = jac_nan();
        for (int i = tid; i < n * Ns; i += T) masks[i] = 0;
        if (tid == 0) a.status[b] = VIB_BAD_INPUT, a.asym[b] = jac_nan();
        return;
    }
    const double two_h = 2.0 * a.h;
    for (size_t i = tid; i < total; i += T) {
        const size_t r = i / W, c = i % W;
        Phi[i] = vib_hessian(Gc[(2 * r) * W + c], Gc[(2 * r + 1) * W + c], two_h);
    }
    __syncthreads();
    double mh = 0.0, md = 0.0;
    for (size_t i = tid; i < total; i += T) {
        const double x = fabs(Phi[i]), y = fabs(Phi[i] - Phi[ph_partner(i, n, Ns, reps)]);
        mh = x > mh ? x : mh, md = y > md ? y : md;
    }
    mh = block_max_f64<PH_THREADS>(mh, red, tid);
    md = block_max_f64<PH_THREADS>(md, red, tid);   // (its first barrier also closes the reads of Phi above)
    if (tid == 0) a.asym[b] = mh > 0.0 ? md / mh : 0.0, a.status[b] = VIB_OK;
    for (size_t i = tid; i < total; i += T) {   // a pair is written by the thread of its lower index
        const size_t p = ph_partner(i, n, Ns, reps);
        if (i < p) Phi[i] = Phi[p] = vib_mean(Phi[i], Phi[p]);
    }
    __syncthreads();
    for (int i = tid; i < 9 * n; i += T) {   // reads the blocks (I, j) != (0, i) only, writes block (0 i; 0 i)
        const int at = i / 9, d = (i % 9) / 3, e = i % 3;
        Phi[(size_t)(3 * at + d) * W + 3 * at + e] = ph_asr(Phi, n, Ns, at, d, e);
    }
    __syncthreads();
    for (int i = tid; i < 9 * n; i += T) {
        const int at = i / 9, d = (i % 9) / 3, e = i % 3;
        if (d < e) {
            double* p = Phi + (size_t)(3 * at + d) * W + 3 * at + e;
            double* q = Phi + (size_t)(3 * at + e) * W + 3 * at + d;
            *p = *q = vib_mean(*p, *q);
        }
    }
    for (int i = tid; i < n * Ns; i += T) masks[i] = ph_mask(frac + 3 * (i / Ns), frac + 3 * (i % Ns), L, a.tie_tol);
}

__global__ __launch_bounds__(PH_THREADS) void phonon_dynmat_kernel(mi_phonon_dynmat_args a) {
    __shared__ double red[PH_THREADS / 64];
    const int t = blockIdx.x, tid = threadIdx.x, T = PH_THREADS;
    const int b = a.item_crystal[t], q = a.item_q[t], M = a.sizes[t];
    if (b < 0 || b >= a.B || q < 0 || q >= a.Q || M < 0 || M > EIG_MAX_M) return;   // (uniform) nothing is addressed through such an item
    const int reps[3] = {a.reps[0], a.reps[1], a.reps[2]};
    const int n0 = a.node_off[b], Ns = a.node_off[b + 1] - n0;
    const int n = ph_prim_atoms(Ns, ph_images(reps), VIB_MAX_ATOMS);
    double* E = a.mats + a.mat_off[t];
    if (n == 0 || M != 6 * n || a.fc_status[b] != VIB_OK) {   // (uniform)
        for (size_t i = tid; i < (size_t)M * M; i += T) E[i] = jac_nan();
        if (tid == 0) a.herm[t] = jac_nan();
        return;
    }
    const int m = 3 * n;
    const size_t total = (size_t)9 * n * Ns;
    const double* Phi = a.workspace + a.ws_off[b] + 2 * total;
    const int* masks = reinterpret_cast<const int*>(a.workspace + a.ws_off[b] + 3 * total);
    const double* tab = a.table + (size_t)q * ph_table_len(reps);
    const double* mass = a.mass + n0;
    for (int i = tid; i < m * m; i += T) {   // A in the upper left block, B in the lower left one
        const int x = i / m, y = i % m;
        double A, B;
        ph_dyn_element(Phi, masks, mass, n, Ns, reps, tab, x, y, &A, &B);
        E[(size_t)x * M + y] = A, E[(size_t)(m + x) * M + y] = B;
    }
    __syncthreads();
    double mh = 0.0, md = 0.0;
    for (int i = tid; i < m * m; i += T) {
        const int x = i / m, y = i % m;
        const double A = E[(size_t)x * M + y], B = E[(size_t)(m + x) * M + y];
        const double da = fabs(A - E[(size_t)y * M + x]), db = fabs(B + E[(size_t)(m + y) * M + x]);
        const double xa = fabs(A), xb = fabs(B);
        mh = xa > mh ? xa : mh, mh = xb > mh ? xb : mh, md = da > md ? da : md, md = db > md ? db : md;
    }
    mh = block_max_f64<PH_THREADS>(mh, red, tid);
    md = block_max_f64<PH_THREADS>(md, red, tid);   // (its first barrier also closes the reads above)
    if (tid == 0) a.herm[t] = mh > 0.0 ? md / mh : 0.0;
    for (int i = tid; i < m * m; i += T) {   // the pair (x, y), x <= y, writes its eight elements of the embedding; no other pair reads them
        const int x = i / m, y = i % m;
        if (x > y) continue;
        const double A = vib_mean(E[(size_t)x * M + y], E[(size_t)y * M + x]);
        if (x == y) {
            E[(size_t)x * M + x] = E[(size_t)(m + x) * M + m + x] = A;
            E[(size_t)(m + x) * M + x] = E[(size_t)x * M + m + x] = 0.0;
            continue;
        }
        const double B = ph_half_diff(E[(size_t)(m + x) * M + y], E[(size_t)(m + y) * M + x]);
        E[(size_t)x * M + y] = E[(size_t)y * M + x] = A;
        E[(size_t)(m + x) * M + m + y] = E[(size_t)(m + y) * M + m + x] = A;
        E[(size_t)(m + x) * M + y] = B, E[(size_t)(m + y) * M + x] = -B;
        E[(size_t)x * M + m + y] = -B, E[(size_t)y * M + m + x] = B;
    }
}

__global__ __launch_bounds__(64) void phonon_thermo_kernel(mi_phonon_thermo_args a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int t0 = a.item_off[b], t1 = a.item_off[b + 1];
    int st = a.fc_status[b];
    const int m = t1 > t0 ? a.sizes[t0] / 2 : 0;
    bool shaped = t1 > t0 && m >= 0;
    for (int t = t0; t < t1; ++t) {
        shaped = shaped && a.sizes[t] == 2 * m && a.item_q[t] >= 0 && a.item_q[t] < a.Q;
        if (st == VIB_OK && a.eig_status[t] > st) st = a.eig_status[t];
    }
    const bool ok = st == VIB_OK && shaped;
    for (int t = t0; t < t1; ++t) {
        const int mt = a.sizes[t] / 2;
        const double* ev = a.evals + a.ev_off[t];
        double* lam = a.lam + a.ev_off[t] / 2;
        double* nu = a.freqs + a.ev_off[t] / 2;
        for (int k = tid; k < mt; k += 64) {
            const double l = ok ? ph_pair_mean(ev, k) : jac_nan();
            lam[k] = l, nu[k] = ok ? vib_frequency(l) : jac_nan();
        }
    }
    __syncthreads();   // (one wave: the lanes below read every lane's lam)
    if (tid < a.K) a.c_v[(size_t)b * a.K + tid] = ok ? ph_cv(a.lam, a.ev_off, a.item_q, a.weight, t0, t1, m, a.nu_cut, a.temps[tid]) : jac_nan();
    if (tid == VIB_MAX_TEMPS) {
        int ni = -1, nz = -1;
        const double z = ok ? ph_zpe(a.lam, a.ev_off, a.item_q, a.weight, t0, t1, m, a.nu_cut, &ni, &nz) : jac_nan();
        a.zpe[b] = z, a.n_imag[b] = ni, a.n_zero[b] = nz, a.status[b] = ok ? VIB_OK : (st == VIB_OK ? VIB_BAD_INPUT : st);
    }
    if (tid == VIB_MAX_TEMPS + 1) {   // pair_gap, herm, sweeps_max
        double hm = 0.0;
        int sw = ok ? 0 : -1;
        for (int t = t0; ok && t < t1; ++t) {
            hm = a.herm_item[t] > hm ? a.herm_item[t] : hm;
            sw = a.sweeps[t] > sw ? a.sweeps[t] : sw;
        }
        a.pair_gap[b] = ok ? ph_pair_gap(a.evals, a.ev_off, t0, t1, m) : jac_nan();
        a.herm[b] = ok ? hm : jac_nan();
        a.sweeps_max[b] = sw;
    }
    if (tid == VIB_MAX_TEMPS + 2) {   // the lowest frequency and the q that has it first
        int at = -1;
        const double lo = ok ? ph_min_freq(a.lam, a.ev_off, a.item_q, t0, t1, m, &at) : jac_nan();
        a.min_freq[b] = lo, a.min_q[b] = at;
    }
}

}  // namespace mi

using namespace mi;

extern "C" {

int64_t mi_phonon_workspace(const int* num_atoms_host, const int* reps_host, int B, int64_t* offsets_host) {
    MI_CHECK(B >= 0 && (num_atoms_host || B == 0) && reps_host, MI_EINVAL, "mi_phonon_workspace: B = %d or a null list", B);
    MI_CHECK(reps_host[0] >= 1 && reps_host[1] >= 1 && reps_host[2] >= 1 && (int64_t)reps_host[0] * reps_host[1] * reps_host[2] <= MI_VIB_MAX_ATOMS, MI_EINVAL,
             "mi_phonon_workspace: reps = (%d, %d, %d): each >= 1, at most %d images", reps_host[0], reps_host[1], reps_host[2], MI_VIB_MAX_ATOMS);
    const int64_t N = (int64_t)reps_host[0] * reps_host[1] * reps_host[2];
    int64_t o = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t Ns = num_atoms_host[b];
        MI_CHECK(Ns >= 1 && Ns <= MI_VIB_MAX_ATOMS, MI_EINVAL, "mi_phonon_workspace: crystal %d has %d atoms (1 .. %d)", b, (int)Ns, MI_VIB_MAX_ATOMS);
        MI_CHECK(Ns % N == 0, MI_EINVAL, "mi_phonon_workspace: crystal %d: reps does not divide the atom count (%d atoms, %d images)", b, (int)Ns, (int)N);
        const int64_t n = Ns / N;
        MI_CHECK(6 * n <= MI_EIG_MAX_M, MI_EINVAL, "mi_phonon_workspace: crystal %d: 6 n > MI_EIG_MAX_M (n = %d, 6 n = %d > %d)", b, (int)n, (int)(6 * n),
                 MI_EIG_MAX_M);
        if (offsets_host) offsets_host[b] = o;
        o += 27 * n * Ns + (n * Ns + 1) / 2;
    }
    if (offsets_host) offsets_host[B] = o;
    return o * (int64_t)sizeof(double);
}

int mi_phonon_fc(const mi_phonon_fc_args* args, void* stream) {
    MI_CHECK(args, MI_EINVAL, "mi_phonon_fc: null argument block");
    const mi_phonon_fc_args& a = *args;
    MI_CHECK(a.B >= 0, MI_EINVAL, "mi_phonon_fc: B = %d", a.B);
    MI_CHECK(pos_finite(a.h) && pos_finite(a.det_min), MI_EINVAL, "mi_phonon_fc: h = %g, det_min = %g: each must be finite and positive", a.h, a.det_min);
    MI_CHECK(std::isfinite(a.tie_tol) && a.tie_tol >= 0.0, MI_EINVAL, "mi_phonon_fc: tie_tol = %g", a.tie_tol);
    MI_CHECK(a.reps[0] >= 1 && a.reps[1] >= 1 && a.reps[2] >= 1 && (int64_t)a.reps[0] * a.reps[1] * a.reps[2] <= MI_VIB_MAX_ATOMS, MI_EINVAL,
             "mi_phonon_fc: reps = (%d, %d, %d): each >= 1, at most %d images", a.reps[0], a.reps[1], a.reps[2], MI_VIB_MAX_ATOMS);
    MI_CHECK(a.max_atoms >= 1 && a.max_atoms <= MI_VIB_MAX_ATOMS, MI_EINVAL, "mi_phonon_fc: max_atoms = %d outside 1..%d", a.max_atoms, MI_VIB_MAX_ATOMS);
    if (a.B == 0) return MI_OK;
    MI_CHECK(a.workspace && a.ws_off && a.node_off && a.mass && a.frac && a.lat && a.asym && a.status, MI_EINVAL, "mi_phonon_fc: null pointer");
    hipLaunchKernelGGL(phonon_fc_kernel, dim3(a.B), dim3(PH_THREADS), 0, (hipStream_t)stream, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int mi_phonon_dynmat(const mi_phonon_dynmat_args* args, void* stream) {
    MI_CHECK(args, MI_EINVAL, "mi_phonon_dynmat: null argument block");
    const mi_phonon_dynmat_args& a = *args;
    MI_CHECK(a.B >= 0 && a.Q >= 0 && a.T >= 0, MI_EINVAL, "mi_phonon_dynmat: B = %d, Q = %d, T = %d", a.B, a.Q, a.T);
    MI_CHECK(a.reps[0] >= 1 && a.reps[1] >= 1 && a.reps[2] >= 1 && (int64_t)a.reps[0] * a.reps[1] * a.reps[2] <= MI_VIB_MAX_ATOMS, MI_EINVAL,
             "mi_phonon_dynmat: reps = (%d, %d, %d): each >= 1, at most %d images", a.reps[0], a.reps[1], a.reps[2], MI_VIB_MAX_ATOMS);
    const int64_t want = (int64_t)a.Q * 6 * (a.reps[0] + a.reps[1] + a.reps[2]);
    MI_CHECK(a.table_len == want, MI_EINVAL, "mi_phonon_dynmat: the q-table has %lld doubles, Q = %d and reps = (%d, %d, %d) need %lld", (long long)a.table_len, a.Q,
             a.reps[0], a.reps[1], a.reps[2], (long long)want);
    if (a.T == 0) return MI_OK;
    MI_CHECK(a.workspace && a.ws_off && a.node_off && a.mass && a.fc_status && a.table && a.item_crystal && a.item_q && a.mats && a.mat_off && a.sizes && a.herm,
             MI_EINVAL, "mi_phonon_dynmat: null pointer");
    hipLaunchKernelGGL(phonon_dynmat_kernel, dim3(a.T), dim3(PH_THREADS), 0, (hipStream_t)stream, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int mi_phonon_thermo(const mi_phonon_thermo_args* args, void* stream) {
    MI_CHECK(args, MI_EINVAL, "mi_phonon_thermo: null argument block");
    const mi_phonon_thermo_args& a = *args;
    MI_CHECK(a.B >= 0 && a.Q >= 0, MI_EINVAL, "mi_phonon_thermo: B = %d, Q = %d", a.B, a.Q);
    MI_CHECK(a.K >= 1 && a.K <= MI_VIB_MAX_TEMPS, MI_EINVAL, "mi_phonon_thermo: K = %d outside 1..%d", a.K, MI_VIB_MAX_TEMPS);
    for (int k = 0; k < a.K; ++k) MI_CHECK(pos_finite(a.temps[k]), MI_EINVAL, "mi_phonon_thermo: temperature %d = %g: must be finite and positive", k, a.temps[k]);
    MI_CHECK(std::isfinite(a.nu_cut) && a.nu_cut >= 0.0, MI_EINVAL, "mi_phonon_thermo: nu_cut = %g", a.nu_cut);
    if (a.B == 0) return MI_OK;
    MI_CHECK(a.evals && a.ev_off && a.sizes && a.eig_status && a.sweeps && a.herm_item && a.fc_status && a.item_off && a.item_q && a.weight && a.lam && a.freqs &&
                 a.c_v && a.zpe && a.n_imag && a.n_zero && a.min_freq && a.min_q && a.herm && a.pair_gap && a.sweeps_max && a.status,
             MI_EINVAL, "mi_phonon_thermo: null pointer");
    hipLaunchKernelGGL(phonon_thermo_kernel, dim3(a.B), dim3(64), 0, (hipStream_t)stream, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // extern "C"
