// The arithmetic of mi_phonon_fc, mi_phonon_dynmat and mi_phonon_thermo (include/matinvent_hip_phonon.h), host and device: the
// force constants of a supercell's home cell from central differences of a learned energy's gradient, their index symmetry and acoustic
// sum rule, the shortest-image table, the dynamical matrix at any q as its real symmetric embedding, and the harmonic thermodynamics of
// a weighted q list.  phonon.hip's kernels call these functions, and scripts/phonon_host_check.cpp runs the same text against plain loops
// under the host sanitizers.  float64 throughout, separately rounded operations: no contraction into FMAs, and NO transcendental function
// (the phases e^{2 pi i q_d r_d} arrive in a host table; sqrt and division are IEEE).  Coordinates and lattices arrive as float32 and are
// widened on read.
//
// Conventions: a primitive cell of n atoms, reps = (a, b, c), N = a b c images I = (I_a b + I_b) c + I_c, a supercell of Ns = n N atoms,
// atom (I, j) at index I n + j.  Phi [3 n][3 Ns] holds Phi(0 i d; I j e) at row 3 i + d, column 3 (I n + j) + e.  Every sum is a serial loop
// in ascending index order, so its order is a function of n and reps alone.
#pragma once
#include "vib_dynmat.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PH_HD __host__ __device__ inline
#else
#define PH_HD inline
#endif

namespace mi {

enum { PH_MAX_PRIM = 128, PH_IMAGES = 27 };

#pragma clang fp contract(off)

PH_HD int ph_images(const int* reps) { return reps[0] * reps[1] * reps[2]; }
PH_HD void ph_decode(int I, const int* reps, int* Ia, int* Ib, int* Ic) {
    *Ic = I % reps[2];
    *Ib = (I / reps[2]) % reps[1];
    *Ia = I / (reps[2] * reps[1]);
}
// the image -I, modulo reps per axis
PH_HD int ph_neg_image(int I, const int* reps) {
    int Ia, Ib, Ic;
    ph_decode(I, reps, &Ia, &Ib, &Ic);
    const int na = (reps[0] - Ia) % reps[0], nb = (reps[1] - Ib) % reps[1], nc = (reps[2] - Ic) % reps[2];
    return (na * reps[1] + nb) * reps[2] + nc;
}
// the element that the index symmetry pairs with element (row 3 i + d, column 3 (I n + j) + e): (row 3 j + e, column 3 ((-I) n + i) + d)
PH_HD size_t ph_partner(size_t idx, int n, int Ns, const int* reps) {
    const size_t W = (size_t)3 * Ns;
    const int row = (int)(idx / W), col = (int)(idx % W);
    const int i = row / 3, d = row % 3, at = col / 3, e = col % 3, I = at / n, j = at % n;
    return (size_t)(3 * j + e) * W + (size_t)3 * (ph_neg_image(I, reps) * n + i) + d;
}

// -sum over (I, j) != (0, i), ascending, of Phi(0 i d; I j e)
PH_HD double ph_asr(const double* Phi, int n, int Ns, int i, int d, int e) {
    double sum = 0.0;
    for (int at = 0; at < Ns; ++at)
        if (at != i) sum += Phi[(size_t)(3 * i + d) * 3 * Ns + 3 * at + e];
    return -sum;
}

// the lattice widened; false: a non-finite element or |det L| < det_min
PH_HD bool ph_lattice(const float* lat, double det_min, double* L) {
    double Li[9];
    for (int q = 0; q < 9; ++q) L[q] = (double)lat[q];
    return vib_lattice(lat, det_min, Li);
}

// |(xj - xi + S) L| for image s = 9 (S_a + 1) + 3 (S_b + 1) + (S_c + 1)
PH_HD double ph_image_dist(const float* xi, const float* xj, int s, const double* L) {
    const double u0 = ((double)xj[0] - (double)xi[0]) + (double)(s / 9 - 1);
    const double u1 = ((double)xj[1] - (double)xi[1]) + (double)((s / 3) % 3 - 1);
    const double u2 = ((double)xj[2] - (double)xi[2]) + (double)(s % 3 - 1);
    const double c0 = (u0 * L[0] + u1 * L[3]) + u2 * L[6];
    const double c1 = (u0 * L[1] + u1 * L[4]) + u2 * L[7];
    const double c2 = (u0 * L[2] + u1 * L[5]) + u2 * L[8];
    return sqrt((c0 * c0 + c1 * c1) + c2 * c2);
}
// the shortest-image mask of a pair of supercell atoms: two passes over the 27 images, nothing kept between them but the minimum
PH_HD int ph_mask(const float* xi, const float* xj, const double* L, double tie_tol) {
    double dmin = ph_image_dist(xi, xj, 0, L);
    for (int s = 1; s < PH_IMAGES; ++s) {
        const double d = ph_image_dist(xi, xj, s, L);
        dmin = d < dmin ? d : dmin;
    }
    const double lim = dmin + tie_tol;
    int mask = 0;
    for (int s = 0; s < PH_IMAGES; ++s) mask |= (ph_image_dist(xi, xj, s, L) <= lim) ? (1 << s) : 0;
    return mask;
}
PH_HD int ph_popcount(int mask) {
    int c = 0;
    for (int s = 0; s < PH_IMAGES; ++s) c += (mask >> s) & 1;
    return c;
}

// entries per q of the phase table (doubles), and the offset of axis d's entry r (r = -reps_d .. 2 reps_d - 1)
PH_HD int ph_table_len(const int* reps) { return 6 * (reps[0] + reps[1] + reps[2]); }
PH_HD int ph_table_at(const int* reps, int d, int r) {
    const int base = d == 0 ? 0 : (d == 1 ? 3 * reps[0] : 3 * (reps[0] + reps[1]));
    return 2 * (base + r + reps[d]);
}

// (1 / mult) sum over the mask's images, ascending, of (t_a t_b) t_c: the phase of image I of one pair
PH_HD void ph_phase(int mask, int I, const int* reps, const double* tab, double* pr, double* pi) {
    int Ia, Ib, Ic;
    ph_decode(I, reps, &Ia, &Ib, &Ic);
    double sr = 0.0, si = 0.0;
    for (int s = 0; s < PH_IMAGES; ++s) {
        if (!((mask >> s) & 1)) continue;
        const double* ta = tab + ph_table_at(reps, 0, Ia + (s / 9 - 1) * reps[0]);
        const double* tb = tab + ph_table_at(reps, 1, Ib + ((s / 3) % 3 - 1) * reps[1]);
        const double* tc = tab + ph_table_at(reps, 2, Ic + (s % 3 - 1) * reps[2]);
        const double ur = ta[0] * tb[0] - ta[1] * tb[1], ui = ta[0] * tb[1] + ta[1] * tb[0];
        sr += ur * tc[0] - ui * tc[1];
        si += ur * tc[1] + ui * tc[0];
    }
    const double mult = (double)ph_popcount(mask);
    *pr = sr / mult, *pi = si / mult;
}

// element (x, y) = ((i, d), (j, e)) of D(q) = A + i B before it is made Hermitian
PH_HD void ph_dyn_element(const double* Phi, const int* masks, const double* mass, int n, int Ns, const int* reps, const double* tab, int x, int y,
                          double* A, double* B) {
    const int i = x / 3, j = y / 3, e = y % 3, N = Ns / n;
    double sr = 0.0, si = 0.0;
    for (int I = 0; I < N; ++I) {
        double pr, pi;
        ph_phase(masks[((size_t)i * N + I) * n + j], I, reps, tab, &pr, &pi);
        const double phi = Phi[(size_t)x * 3 * Ns + 3 * (I * n + j) + e];
        sr += phi * pr;
        si += phi * pi;
    }
    *A = vib_mass_weight(sr, mass[i], mass[j]);
    *B = vib_mass_weight(si, mass[i], mass[j]);
}
PH_HD double ph_half_diff(double a, double b) { return (a - b) * 0.5; }

// ---- thermodynamics of one crystal's items ---------------------------------------------------------------------------------------------

PH_HD double ph_pair_mean(const double* ev, int k) { return vib_mean(ev[2 * k], ev[2 * k + 1]); }

// c_v / k_B at T per primitive cell: sum_q w_q vib_cv(lambda of q) / sum_q w_q, the items in order
PH_HD double ph_cv(const double* lam, const int64_t* ev_off, const int* item_q, const int* weight, int t0, int t1, int m, double nu_cut, double T) {
    double s = 0.0, wsum = 0.0;
    for (int t = t0; t < t1; ++t) {
        const double w = (double)weight[item_q[t]];
        s += w * vib_cv(lam + ev_off[t] / 2, m, nu_cut, T);
        wsum += w;
    }
    return s / wsum;
}
PH_HD double ph_zpe(const double* lam, const int64_t* ev_off, const int* item_q, const int* weight, int t0, int t1, int m, double nu_cut, int* n_imag,
                    int* n_zero) {
    double s = 0.0, wsum = 0.0;
    int ni = 0, nz = 0;
    for (int t = t0; t < t1; ++t) {
        const int w = weight[item_q[t]];
        int a, b;
        s += (double)w * vib_zpe(lam + ev_off[t] / 2, m, nu_cut, &a, &b);
        wsum += (double)w;
        ni += w * a, nz += w * b;
    }
    *n_imag = ni, *n_zero = nz;
    return s / wsum;
}

// max (ev[2 k + 1] - ev[2 k]) / max |ev| over a crystal's items: the embedding's own check
PH_HD double ph_pair_gap(const double* evals, const int64_t* ev_off, int t0, int t1, int m) {
    double gap = 0.0, top = 0.0;
    for (int t = t0; t < t1; ++t) {
        const double* ev = evals + ev_off[t];
        for (int k = 0; k < m; ++k) {
            const double g = ev[2 * k + 1] - ev[2 * k], x = fabs(ev[2 * k]), y = fabs(ev[2 * k + 1]);
            gap = g > gap ? g : gap, top = x > top ? x : top, top = y > top ? y : top;
        }
    }
    return top > 0.0 ? gap / top : 0.0;
}
// the lowest frequency of a crystal's items and the q that has it first (-1 and NaN: no mode)
PH_HD double ph_min_freq(const double* lam, const int64_t* ev_off, const int* item_q, int t0, int t1, int m, int* q_at) {
    double lo = jac_nan();
    int at = -1;
    for (int t = t0; t < t1; ++t)
        for (int k = 0; k < m; ++k) {
            const double nu = vib_frequency(lam[ev_off[t] / 2 + k]);
            if (at < 0 || nu < lo) lo = nu, at = item_q[t];
        }
    *q_at = at;
    return lo;
}

// ---- one crystal, serially (the host check's form; the kernels spread the same element functions over a workgroup) ---------------------

// Gc [6 n][3 Ns], mass [n] (the home cell's), frac [Ns][3], lat [9] -> Phi [3 n][3 Ns], masks [n][N][n], asym.  Returns the status.
inline int ph_fc_crystal_host(int Ns, const int* reps, const double* Gc, const double* mass, const float* frac, const float* lat, double h, double tie_tol,
                              double det_min, double* Phi, int* masks, double* asym) {
    const int N = ph_images(reps);
    if (Ns < 1 || Ns > VIB_MAX_ATOMS || Ns % N != 0 || Ns / N > PH_MAX_PRIM) {
        *asym = jac_nan();
        return VIB_BAD_INPUT;
    }
    const int n = Ns / N;
    const size_t W = (size_t)3 * Ns, total = (size_t)3 * n * W;
    double L[9];
    bool ok = ph_lattice(lat, det_min, L);
    for (size_t i = 0; i < 2 * total; ++i) ok = ok && jac_finite(Gc[i]);
    for (int j = 0; j < n; ++j) ok = ok && jac_finite(mass[j]) && mass[j] > 0.0;
    if (!ok) {
        for (size_t i = 0; i < total; ++i) Phi[i] = jac_nan();
        for (size_t i = 0; i < (size_t)n * Ns; ++i) masks[i] = 0;
        *asym = jac_nan();
        return VIB_BAD_INPUT;
    }
    const double two_h = 2.0 * h;
    for (size_t idx = 0; idx < total; ++idx) {
        const size_t r = idx / W, c = idx % W;
        Phi[idx] = vib_hessian(Gc[(2 * r) * W + c], Gc[(2 * r + 1) * W + c], two_h);
    }
    double mh = 0.0, md = 0.0;
    for (size_t idx = 0; idx < total; ++idx) {
        const double x = fabs(Phi[idx]), y = fabs(Phi[idx] - Phi[ph_partner(idx, n, Ns, reps)]);
        mh = x > mh ? x : mh, md = y > md ? y : md;
    }
    *asym = mh > 0.0 ? md / mh : 0.0;
    for (size_t idx = 0; idx < total; ++idx) {   // the pair is written from its lower index
        const size_t p = ph_partner(idx, n, Ns, reps);
        if (idx < p) Phi[idx] = Phi[p] = vib_mean(Phi[idx], Phi[p]);
    }
    for (int i = 0; i < n; ++i) {
        double blk[9];
        for (int d = 0; d < 3; ++d)
            for (int e = 0; e < 3; ++e) blk[3 * d + e] = ph_asr(Phi, n, Ns, i, d, e);
        for (int d = 0; d < 3; ++d)
            for (int e = 0; e < 3; ++e) Phi[(size_t)(3 * i + d) * W + 3 * i + e] = vib_mean(blk[3 * d + e], blk[3 * e + d]);
    }
    for (int i = 0; i < n; ++i)
        for (int at = 0; at < Ns; ++at) masks[((size_t)i * N + at / n) * n + at % n] = ph_mask(frac + 3 * i, frac + 3 * at, L, tie_tol);
    return VIB_OK;
}

// the embedding E [6 n][6 n] of D(q) and herm, from Phi, the masks and one q's table
inline void ph_dynmat_item_host(int n, int Ns, const int* reps, const double* Phi, const int* masks, const double* mass, const double* tab, double* E,
                                double* herm) {
    const int m = 3 * n, M = 2 * m;
    for (int x = 0; x < m; ++x)
        for (int y = 0; y < m; ++y) ph_dyn_element(Phi, masks, mass, n, Ns, reps, tab, x, y, &E[(size_t)x * M + y], &E[(size_t)(m + x) * M + y]);
    double mh = 0.0, md = 0.0;
    for (int x = 0; x < m; ++x)
        for (int y = 0; y < m; ++y) {
            const double a = E[(size_t)x * M + y], b = E[(size_t)(m + x) * M + y];
            const double da = fabs(a - E[(size_t)y * M + x]), db = fabs(b + E[(size_t)(m + y) * M + x]);
            const double xa = fabs(a), xb = fabs(b);
            mh = xa > mh ? xa : mh, mh = xb > mh ? xb : mh, md = da > md ? da : md, md = db > md ? db : md;
        }
    *herm = mh > 0.0 ? md / mh : 0.0;
    for (int x = 0; x < m; ++x)
        for (int y = x; y < m; ++y) {
            const double a = vib_mean(E[(size_t)x * M + y], E[(size_t)y * M + x]);
            if (x == y) {   // (a real diagonal)
                E[(size_t)x * M + x] = E[(size_t)(m + x) * M + m + x] = a;
                E[(size_t)(m + x) * M + x] = E[(size_t)x * M + m + x] = 0.0;
                continue;
            }
            const double b = ph_half_diff(E[(size_t)(m + x) * M + y], E[(size_t)(m + y) * M + x]);
            E[(size_t)x * M + y] = E[(size_t)y * M + x] = a;
            E[(size_t)(m + x) * M + m + y] = E[(size_t)(m + y) * M + m + x] = a;
            E[(size_t)(m + x) * M + y] = b, E[(size_t)(m + y) * M + x] = -b;
            E[(size_t)x * M + m + y] = -b, E[(size_t)y * M + m + x] = b;
        }
}

}  // namespace mi
