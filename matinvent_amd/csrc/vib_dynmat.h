// The arithmetic of mi_vib_displace, mi_vib_collect, mi_vib_dynmat and mi_vib_thermo (include/matinvent_hip_vib.h), host and
// device: the Gamma-point dynamical matrix of one crystal from central differences of a learned energy's gradient, its reduction to the
// vibrational block, and the harmonic thermodynamics of its eigenvalues.  vib.hip's kernels call these functions, and
// scripts/vib_host_check.cpp runs the same text against plain loops under the host sanitizers.  float64 throughout, separately rounded
// operations: no contraction into FMAs.  Gradients, coordinates and lattices arrive as float32 and are widened on read.
//
// Conventions (relax_fire.h's): lattice rows are cell vectors, cart = frac L, dE / dr_j = g_frac[j] L^-T, d frac = dr L^-1.  A crystal of n
// atoms has N3 = 3 n Cartesian degrees of freedom a = 3 i + d and 6 n displaced copies c = 2 a + s (s = 0: +h, s = 1: -h).  Every sum is a
// serial loop in ascending index order, so its order is a function of n alone.
#pragma once
#include "guide_shift.h"
#include "sym_jacobi.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VIB_HD __host__ __device__ inline
#else
#define VIB_HD inline
#endif

namespace mi {

enum { VIB_OK = 0, VIB_NO_CONVERGENCE = 1, VIB_BAD_INPUT = 2 };
enum { VIB_MAX_ATOMS = 256, VIB_MAX_TEMPS = 8 };
// nu = sqrt(lambda) / (2 pi) for lambda in eV / (amu A^2):  sqrt(e / (u 1e-20 m^2)) / (2 pi) with CODATA 2018 e = 1.602176634e-19 C (exact) and
// u = 1.66053906660e-27 kg  ->  1.5633304e13 Hz
constexpr double VIB_THZ = 15.633304;
// h = 6.62607015e-34 J s, k_B = 1.380649e-23 J / K, e as above (all exact):  h / e x 1e12 Hz and h x 1e12 Hz / k_B
constexpr double VIB_H_EV_THZ = 4.135667696923859e-3;   // eV per THz
constexpr double VIB_H_KB_THZ = 47.992430733662204;     // K per THz
constexpr double VIB_X_MAX = 700.0;                     // a mode with h nu / (k_B T) above it contributes exactly 0 to c_v

#pragma clang fp contract(off)

VIB_HD int vib_modes(int n) { return 3 * n - 3; }

// relax_fire.h's determinant and cofactor inverse, in float64
VIB_HD double vib_det3(const double* L) {
    const double c0 = L[4] * L[8] - L[5] * L[7], c1 = L[5] * L[6] - L[3] * L[8], c2 = L[3] * L[7] - L[4] * L[6];
    return (L[0] * c0 + L[1] * c1) + L[2] * c2;
}
VIB_HD void vib_inv3(const double* L, double det, double* Li) {
    Li[0] = (L[4] * L[8] - L[5] * L[7]) / det;
    Li[1] = (L[2] * L[7] - L[1] * L[8]) / det;
    Li[2] = (L[1] * L[5] - L[2] * L[4]) / det;
    Li[3] = (L[5] * L[6] - L[3] * L[8]) / det;
    Li[4] = (L[0] * L[8] - L[2] * L[6]) / det;
    Li[5] = (L[2] * L[3] - L[0] * L[5]) / det;
    Li[6] = (L[3] * L[7] - L[4] * L[6]) / det;
    Li[7] = (L[1] * L[6] - L[0] * L[7]) / det;
    Li[8] = (L[0] * L[4] - L[1] * L[3]) / det;
}
// the lattice widened; false: a non-finite element or |det L| < det_min (Li is not written)
VIB_HD bool vib_lattice(const float* lat, double det_min, double* Li) {
    double L[9];
    bool ok = true;
    for (int q = 0; q < 9; ++q) {
        ok = ok && guide_finite(lat[q]);
        L[q] = (double)lat[q];
    }
    if (!ok) return false;
    const double det = vib_det3(L);
    if (!(fabs(det) >= det_min)) return false;
    vib_inv3(L, det, Li);
    return true;
}

// component k of the displaced atom of copy c = 2 (3 i + d) + s: frac + (+-h) e_d L^-1, rounded to float32, wrapped
VIB_HD float vib_displaced(float x, double h, int d, int s, int k, const double* Li) {
    const double hs = s ? -h : h;
    return guide_mod1((float)((double)x + hs * Li[3 * d + k]));
}

VIB_HD double vib_scale(double scale, int per_atom, int n) { return per_atom ? scale * (double)n : scale; }   // s_b

// component k of dE / dr_j = s g_frac[j] L^-T
VIB_HD double vib_cart_grad(const float* g, const double* Li, double s, int k) {
    return s * (((double)g[0] * Li[3 * k] + (double)g[1] * Li[3 * k + 1]) + (double)g[2] * Li[3 * k + 2]);
}

VIB_HD double vib_hessian(double gp, double gm, double two_h) { return (gp - gm) / two_h; }
VIB_HD double vib_mean(double a, double b) { return (a + b) * 0.5; }
VIB_HD double vib_mass_weight(double hab, double mi, double mj) { return hab / sqrt(mi * mj); }

// -sum over j != i (ascending) of H[(i, d)][(j, e)]
VIB_HD double vib_asr(const double* W, int N3, int n, int i, int d, int e) {
    double sum = 0.0;
    for (int j = 0; j < n; ++j)
        if (j != i) sum += W[(size_t)(3 * i + d) * N3 + 3 * j + e];
    return -sum;
}

// The three Householder vectors v [3][N3] (unit length, v_k zero above row k) whose reflectors P_k = I - 2 v_k v_k^T, applied in the
// order k = 0, 1, 2, take the normalised translations T[3 j + d][d] = sqrt(m_j / sum m) to multiples of the first three unit vectors.
// Serial: one thread of the kernel.  U [3][N3] is work.
VIB_HD void vib_householder(const double* mass, int n, double* v, double* U) {
    const int N3 = 3 * n;
    double mtot = 0.0;
    for (int j = 0; j < n; ++j) mtot += mass[j];
    const double rt = sqrt(mtot);
    for (int d = 0; d < 3; ++d)
        for (int a = 0; a < N3; ++a) U[d * N3 + a] = (a % 3 == d) ? sqrt(mass[a / 3]) / rt : 0.0;
    for (int k = 0; k < 3; ++k) {
        double* x = U + k * N3;
        double* vk = v + k * N3;
        double nn = 0.0;
        for (int a = k; a < N3; ++a) nn += x[a] * x[a];
        const double alpha = x[k] > 0.0 ? -sqrt(nn) : sqrt(nn);
        for (int a = 0; a < N3; ++a) vk[a] = a < k ? 0.0 : x[a];
        vk[k] = vk[k] - alpha;
        double vn = 0.0;
        for (int a = k; a < N3; ++a) vn += vk[a] * vk[a];
        const double rv = sqrt(vn);
        for (int a = k; a < N3; ++a) vk[a] = vk[a] / rv;
        for (int c = k + 1; c < 3; ++c) {
            double* y = U + c * N3;
            double dot = 0.0;
            for (int a = k; a < N3; ++a) dot += vk[a] * y[a];
            for (int a = k; a < N3; ++a) y[a] = y[a] - (2.0 * dot) * vk[a];
        }
    }
}

// row a of w = D v, and K = v . w
VIB_HD double vib_row_dot(const double* W, int N3, int a, const double* v) {
    double s = 0.0;
    for (int b = 0; b < N3; ++b) s += W[(size_t)a * N3 + b] * v[b];
    return s;
}
VIB_HD double vib_dot(const double* v, const double* w, int N3) {
    double s = 0.0;
    for (int a = 0; a < N3; ++a) s += v[a] * w[a];
    return s;
}
// element (a, b) of P D P = D - 2 v w^T - 2 w v^T + 4 K v v^T
VIB_HD double vib_reflect(double dab, double va, double vb, double wa, double wb, double K) {
    return ((dab - (2.0 * va) * wb) - (2.0 * wa) * vb) + ((4.0 * K) * va) * vb;
}

// ---- thermodynamics of one crystal's eigenvalues --------------------------------------------------------------------------------------

VIB_HD double vib_frequency(double lam) { return lam < 0.0 ? -(sqrt(-lam) * VIB_THZ) : sqrt(lam) * VIB_THZ; }   // THz, negative: imaginary
// 0: contributes, 1: imaginary, 2: zero
VIB_HD int vib_mode_class(double nu, double nu_cut) { return nu < -nu_cut ? 1 : (fabs(nu) <= nu_cut ? 2 : 0); }
// x^2 e^-x / (1 - e^-x)^2 = (x / (e^x - 1)) (x / (1 - e^-x)), x = h nu / (k_B T) > 0
VIB_HD double vib_cv_term(double nu, double T) {
    const double x = (nu * VIB_H_KB_THZ) / T;
    if (!(x < VIB_X_MAX)) return 0.0;
    return (x / expm1(x)) * (x / -expm1(-x));
}
// c_v / k_B at T, the zero-point energy (eV) and the counts from ascending eigenvalues; only real modes above nu_cut contribute
VIB_HD double vib_cv(const double* lam, int M, double nu_cut, double T) {
    double s = 0.0;
    for (int k = 0; k < M; ++k) {
        const double nu = vib_frequency(lam[k]);
        if (vib_mode_class(nu, nu_cut) == 0) s += vib_cv_term(nu, T);
    }
    return s;
}
VIB_HD double vib_zpe(const double* lam, int M, double nu_cut, int* n_imag, int* n_zero) {
    double s = 0.0;
    int ni = 0, nz = 0;
    for (int k = 0; k < M; ++k) {
        const double nu = vib_frequency(lam[k]);
        const int cls = vib_mode_class(nu, nu_cut);
        if (cls == 0) s += nu * VIB_H_EV_THZ;
        ni += cls == 1, nz += cls == 2;
    }
    *n_imag = ni, *n_zero = nz;
    return 0.5 * s;
}

// ---- one crystal, serially (the host check's form; the kernel spreads the same element functions over a workgroup) ---------------------

// Gc [6 n][3 n], mass [n] -> R [M][M] (M = 3 n - 3), asym; W [3 n][3 n], v, U [3][3 n], w [3 n] are work.  Returns the status.
inline int vib_dynmat_crystal_host(int n, const double* Gc, const double* mass, double h, double* R, double* asym, double* W, double* v,
                                   double* U, double* w) {
    const int N3 = 3 * n, M = vib_modes(n);
    bool ok = true;
    for (size_t i = 0; i < (size_t)6 * n * N3; ++i) ok = ok && jac_finite(Gc[i]);
    for (int j = 0; j < n; ++j) ok = ok && jac_finite(mass[j]) && mass[j] > 0.0;
    if (!ok) {
        for (size_t i = 0; i < (size_t)M * M; ++i) R[i] = jac_nan();
        *asym = jac_nan();
        return VIB_BAD_INPUT;
    }
    const double two_h = 2.0 * h;
    for (int a = 0; a < N3; ++a)
        for (int b = 0; b < N3; ++b) W[(size_t)a * N3 + b] = vib_hessian(Gc[(size_t)(2 * a) * N3 + b], Gc[(size_t)(2 * a + 1) * N3 + b], two_h);
    double mh = 0.0, md = 0.0;
    for (int a = 0; a < N3; ++a)
        for (int b = 0; b < N3; ++b) {
            const double x = fabs(W[(size_t)a * N3 + b]), y = fabs(W[(size_t)a * N3 + b] - W[(size_t)b * N3 + a]);
            mh = x > mh ? x : mh, md = y > md ? y : md;
        }
    *asym = mh > 0.0 ? md / mh : 0.0;
    for (int a = 0; a < N3; ++a)
        for (int b = a + 1; b < N3; ++b) W[(size_t)a * N3 + b] = W[(size_t)b * N3 + a] = vib_mean(W[(size_t)a * N3 + b], W[(size_t)b * N3 + a]);
    for (int i = 0; i < n; ++i) {
        double blk[9];
        for (int d = 0; d < 3; ++d)
            for (int e = 0; e < 3; ++e) blk[3 * d + e] = vib_asr(W, N3, n, i, d, e);
        for (int d = 0; d < 3; ++d)
            for (int e = 0; e < 3; ++e) W[(size_t)(3 * i + d) * N3 + 3 * i + e] = vib_mean(blk[3 * d + e], blk[3 * e + d]);   // (a + b is b + a, bit for bit)
    }
    for (int a = 0; a < N3; ++a)
        for (int b = 0; b < N3; ++b) W[(size_t)a * N3 + b] = vib_mass_weight(W[(size_t)a * N3 + b], mass[a / 3], mass[b / 3]);
    if (M == 0) return VIB_OK;
    vib_householder(mass, n, v, U);
    for (int k = 0; k < 3; ++k) {
        const double* vk = v + k * N3;
        for (int a = 0; a < N3; ++a) w[a] = vib_row_dot(W, N3, a, vk);
        const double K = vib_dot(vk, w, N3);
        for (int a = 0; a < N3; ++a)
            for (int b = 0; b < N3; ++b) W[(size_t)a * N3 + b] = vib_reflect(W[(size_t)a * N3 + b], vk[a], vk[b], w[a], w[b], K);
    }
    for (int x = 0; x < M; ++x)
        for (int y = 0; y < M; ++y) R[(size_t)x * M + y] = vib_mean(W[(size_t)(3 + x) * N3 + 3 + y], W[(size_t)(3 + y) * N3 + 3 + x]);
    return VIB_OK;
}

}  // namespace mi
