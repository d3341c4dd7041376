// The arithmetic of mi_elastic_strain, mi_elastic_collect and mi_elastic_fit (include/matinvent_hip_elastic.h), host and device:
// the strained copies of a cell, the Cauchy stress of a copy from the learned energy's lattice gradient, and the elastic tensor, its inverse,
// the Voigt / Reuss / Hill moduli and the eigenvalues of one crystal from the stresses of its 13 copies.  elastic.hip's kernels call these
// functions, and scripts/elastic_host_check.cpp runs the same text under the host sanitizers.  float64 throughout, separately rounded
// operations: no contraction into FMAs.  Gradients and lattices arrive as float32 and are widened on read.
//
// Conventions (relax_fire.h's): lattice rows are cell vectors, cart = frac L, G = s dE / dL as a 3 x 3 matrix.  Copy c = 2 j + s (j = 0 .. 5,
// s = 0: +h, s = 1: -h) carries the strain eps = +-h E_j, E_j = e_j e_j^T (j < 3) or (e_a e_b^T + e_b e_a^T) / 2 for the shear pairs
// (a, b) = (1, 2), (0, 2), (0, 1): Voigt order 11, 22, 33, 23, 13, 12, engineering shear strain exactly h.  Copy 12 is unstrained.  Every
// sum is a serial loop in a fixed order.
#pragma once
#include "relax_fire.h"
#include "vib_dynmat.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ELA_HD __host__ __device__ inline
#else
#define ELA_HD inline
#endif

namespace mi {

enum { ELASTIC_OK = 0, ELASTIC_BAD_INPUT = 1, ELASTIC_SINGULAR = 2 };
enum { ELASTIC_COPIES = 13, ELASTIC_ROW = 8 };   // a workspace row: sigma [6] (eV / A^3), V', flag (1: the copy's ion relaxation was EXHAUSTED)
enum { ELASTIC_VOIGT = 0, ELASTIC_REUSS = 1, ELASTIC_HILL = 2 };
enum { ELASTIC_K = 0, ELASTIC_G = 1, ELASTIC_E = 2, ELASTIC_NU = 3, ELASTIC_PUGH = 4 };   // the columns of moduli [3][5]
enum { ELASTIC_WORK = 36 + 72 + 12 + 6 };   // doubles of work of elastic_fit_crystal: the rotated copy, the augmented matrix, the rotations of a round
// 1 eV / A^3 in GPa: e / 1e-30 m^3 / 1e9 Pa with the SI value e = 1.602176634e-19 C (exact)
constexpr double ELASTIC_GPA = 160.2176634;

#pragma clang fp contract(off)

// the two axes of Voigt component i: (i, i) for i < 3, then (1, 2), (0, 2), (0, 1)
ELA_HD int ela_axis_a(int i) { return i < 3 ? i : (i == 3 ? 1 : 0); }
ELA_HD int ela_axis_b(int i) { return i < 3 ? i : (i == 5 ? 1 : 2); }

// element (r, q) of the strained lattice L (I + eps) of copy c, formed in float64 and rounded once; an element the strain does not reach,
// and every element of copy 12, keeps its bits
ELA_HD float ela_strained(const float* lat, double h, int c, int r, int q) {
    if (c >= 12) return lat[3 * r + q];
    const int j = c >> 1, a = ela_axis_a(j), b = ela_axis_b(j);
    if (q != a && q != b) return lat[3 * r + q];
    const double hs = (c & 1) ? -h : h;
    const double e = a == b ? hs : 0.5 * hs;   // eps[k][q] of the one k that reaches column q
    const int k = q == a ? b : a;
    return (float)((double)lat[3 * r + q] + (double)lat[3 * r + k] * e);
}

// One row of the workspace from a copy's lattice (as the network saw it) and lattice gradient: T = L^T G, sigma = (T + T^T) / (2 V),
// V = |det L|.  *asym = max |T - T^T| / max |T| (0 when T = 0).  false: the lattice is bad and row and asym are NaN.
ELA_HD bool ela_stress_row(const float* lat, const float* g_lat, double s, double det_min, double* row, double* asym) {
    double Li[9];
    if (!vib_lattice(lat, det_min, Li)) {
        for (int i = 0; i < ELASTIC_ROW; ++i) row[i] = jac_nan();
        *asym = jac_nan();
        return false;
    }
    double L[9], G[9], T[9];
    for (int q = 0; q < 9; ++q) L[q] = (double)lat[q], G[q] = s * (double)g_lat[q];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) T[3 * i + j] = (L[i] * G[j] + L[3 + i] * G[3 + j]) + L[6 + i] * G[6 + j];
    const double V = fabs(vib_det3(L)), V2 = 2.0 * V;
    row[0] = (T[0] + T[0]) / V2, row[1] = (T[4] + T[4]) / V2, row[2] = (T[8] + T[8]) / V2;
    row[3] = (T[5] + T[7]) / V2, row[4] = (T[2] + T[6]) / V2, row[5] = (T[1] + T[3]) / V2;
    row[6] = V, row[7] = 0.0;
    double mt = 0.0, md = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double x = fabs(T[3 * i + j]), y = fabs(T[3 * i + j] - T[3 * j + i]);
            mt = x > mt ? x : mt, md = y > md ? y : md;   // (a NaN never enters: the row is then not finite and the fit answers BAD_INPUT)
        }
    *asym = mt > 0.0 ? md / mt : 0.0;
    return true;
}

// The row of one copy as mi_elastic_collect writes it.  ist: the status of the copy's ion relaxation, RELAX_CONVERGED when the ions are
// clamped.  RELAX_FAILED: a row of NaN;  RELAX_EXHAUSTED: the flag is 1.
ELA_HD void ela_collect_row(const float* lat, const float* g_lat, double s, double det_min, int ist, double* row, double* asym) {
    const bool ok = ela_stress_row(lat, g_lat, s, det_min, row, asym);
    if (ist == RELAX_FAILED) {
        for (int i = 0; i < ELASTIC_ROW; ++i) row[i] = jac_nan();
        *asym = jac_nan();
    } else if (ok && ist == RELAX_EXHAUSTED) {
        row[ELASTIC_ROW - 1] = 1.0;
    }
}

ELA_HD double ela_cij(double sp, double sm, double two_h) { return ((sp - sm) / two_h) * ELASTIC_GPA; }

// S = C^-1 by Gauss-Jordan elimination with partial pivoting (the largest |element| of the column at or below the diagonal, ties to the
// lowest row) on the augmented matrix aug [6][12].  false: a zero or non-finite pivot (S is then NaN).
ELA_HD bool ela_invert6(const double* Cm, double* S, double* aug) {
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 12; ++j) aug[12 * i + j] = j < 6 ? Cm[6 * i + j] : (j - 6 == i ? 1.0 : 0.0);
    bool ok = true;
    for (int k = 0; k < 6 && ok; ++k) {
        int piv = k;
        double best = fabs(aug[12 * k + k]);
        for (int r = k + 1; r < 6; ++r) {
            const double v = fabs(aug[12 * r + k]);
            if (v > best) best = v, piv = r;
        }
        const double p = aug[12 * piv + k];
        if (!jac_finite(p) || p == 0.0) {
            ok = false;
            break;
        }
        if (piv != k)
            for (int j = 0; j < 12; ++j) {
                const double t = aug[12 * k + j];
                aug[12 * k + j] = aug[12 * piv + j], aug[12 * piv + j] = t;
            }
        for (int j = 0; j < 12; ++j) aug[12 * k + j] = aug[12 * k + j] / p;
        for (int i = 0; i < 6; ++i) {
            if (i == k) continue;
            const double f = aug[12 * i + k];
            for (int j = 0; j < 12; ++j) aug[12 * i + j] = aug[12 * i + j] - f * aug[12 * k + j];
        }
    }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) S[6 * i + j] = ok ? aug[12 * i + 6 + j] : jac_nan();
    return ok;
}

// Young's modulus, Poisson's ratio and the Pugh ratio of one average from its K and G
ELA_HD void ela_derived(double* m) {
    const double K = m[ELASTIC_K], G = m[ELASTIC_G], d = 3.0 * K + G;
    m[ELASTIC_E] = ((9.0 * K) * G) / d;
    m[ELASTIC_NU] = (3.0 * K - 2.0 * G) / (2.0 * d);
    m[ELASTIC_PUGH] = K / G;
}

// the trace of the upper-left block, the sum of its three off-diagonal elements and the trace of the shear block
ELA_HD void ela_sums(const double* M, double* a, double* b, double* c) {
    *a = (M[0] + M[7]) + M[14];
    *b = (M[1] + M[2]) + M[8];
    *c = (M[21] + M[28]) + M[35];
}

// moduli [3][5] (GPa; nu and K / G are numbers) from C and, when has_S, S; without S the Reuss and Hill rows are NaN
ELA_HD void ela_moduli(const double* Cm, const double* S, bool has_S, double* moduli) {
    double a, b, c;
    ela_sums(Cm, &a, &b, &c);
    double* V = moduli + 5 * ELASTIC_VOIGT;
    double* R = moduli + 5 * ELASTIC_REUSS;
    double* H = moduli + 5 * ELASTIC_HILL;
    V[ELASTIC_K] = (a + 2.0 * b) / 9.0;
    V[ELASTIC_G] = ((a - b) + 3.0 * c) / 15.0;
    ela_derived(V);
    if (!has_S) {
        for (int i = 0; i < 5; ++i) R[i] = H[i] = jac_nan();
        return;
    }
    ela_sums(S, &a, &b, &c);
    R[ELASTIC_K] = 1.0 / (a + 2.0 * b);
    R[ELASTIC_G] = 15.0 / ((4.0 * a - 4.0 * b) + 3.0 * c);
    ela_derived(R);
    H[ELASTIC_K] = (V[ELASTIC_K] + R[ELASTIC_K]) * 0.5;
    H[ELASTIC_G] = (V[ELASTIC_G] + R[ELASTIC_G]) * 0.5;
    ela_derived(H);
}

// sym_jacobi.h's iteration on one matrix of order 6, serially, with its work in caller-given arrays: A [36] is destroyed, rot [12] holds a
// round's three rotations (c, s, pp, qq each).  The element formulas, their order inside a round and the ranking are mi_sym_eigvals':
// the same bits.  Returns the sweeps that rotated, or -1 when A is not finite (ev is NaN).
ELA_HD int ela_eigvals6(double* A, double* ev, double* rot) {
    const int M = 6, np = 3;
    for (int i = 0; i < M * M; ++i)
        if (!jac_finite(A[i])) {
            for (int k = 0; k < M; ++k) ev[k] = jac_nan();
            return -1;
        }
    int done = 0;
    for (int sw = 0; sw < EIG_MAX_SWEEPS; ++sw) {
        int any_sweep = 0;
        for (int r = 0; r < M - 1; ++r) {
            int any = 0, mask = 0, p, q;
            for (int k = 0; k < np; ++k) {
                jac_pair(M, r, k, &p, &q);
                const JacRot R = jac_rotation(A[p * M + p], A[q * M + q], A[p * M + q]);
                rot[4 * k] = R.c, rot[4 * k + 1] = R.s, rot[4 * k + 2] = R.pp, rot[4 * k + 3] = R.qq;
                mask |= R.rot << k, any |= R.rot;
            }
            if (!any) continue;
            any_sweep = 1;
            for (int k = 0; k < np; ++k) {
                if (!((mask >> k) & 1)) continue;
                jac_pair(M, r, k, &p, &q);
                for (int i = 0; i < M; ++i) {
                    const double x = A[i * M + p], y = A[i * M + q];
                    A[i * M + p] = jac_first(rot[4 * k], rot[4 * k + 1], x, y);
                    A[i * M + q] = jac_second(rot[4 * k], rot[4 * k + 1], x, y);
                }
            }
            for (int k = 0; k < np; ++k) {
                if (!((mask >> k) & 1)) continue;
                jac_pair(M, r, k, &p, &q);
                for (int j = 0; j < M; ++j) {
                    const double x = A[p * M + j], y = A[q * M + j];
                    A[p * M + j] = j == p ? rot[4 * k + 2] : (j == q ? 0.0 : jac_first(rot[4 * k], rot[4 * k + 1], x, y));
                    A[q * M + j] = j == q ? rot[4 * k + 3] : (j == p ? 0.0 : jac_second(rot[4 * k], rot[4 * k + 1], x, y));
                }
            }
        }
        if (!any_sweep) break;
        ++done;
    }
    for (int i = 0; i < M; ++i) ev[jac_rank(A, M, M, i)] = A[i * M + i];
    return done;
}

struct ElasticFit {   // the outputs of one crystal
    double* C;        // [36] GPa, symmetrised
    double* S;        // [36] 1 / GPa
    double* stress0;  // [6] GPa
    double* moduli;   // [3][5]
    double* evals;    // [6] GPa, ascending
    double pressure, asym_C, cond;
    int n_negative, n_unrelaxed, status;
};

// One crystal from its 13 workspace rows; work [ELASTIC_WORK].  Serial: one thread of the kernel.  `asym` is the collect step's figure of
// copy 12 and is not read here: the caller blanks it when the status is ELASTIC_BAD_INPUT.
ELA_HD void ela_fit_crystal(const double* rows, double h, double* work, ElasticFit* o) {
    double* A = work;
    double* aug = work + 36;
    double* rot = work + 36 + 72;
    double* ev = work + 36 + 72 + 12;
    bool ok = true;
    int unrelaxed = 0;
    for (int i = 0; i < ELASTIC_COPIES * ELASTIC_ROW; ++i) ok = ok && jac_finite(rows[i]);
    for (int c = 0; c < ELASTIC_COPIES; ++c) unrelaxed += rows[ELASTIC_ROW * c + 7] != 0.0 ? 1 : 0;
    if (!ok) {
        for (int i = 0; i < 36; ++i) o->C[i] = o->S[i] = jac_nan();
        for (int i = 0; i < 6; ++i) o->stress0[i] = o->evals[i] = jac_nan();
        for (int i = 0; i < 15; ++i) o->moduli[i] = jac_nan();
        o->pressure = o->asym_C = o->cond = jac_nan();
        o->n_negative = o->n_unrelaxed = -1, o->status = ELASTIC_BAD_INPUT;
        return;
    }
    const double two_h = 2.0 * h;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) A[6 * i + j] = ela_cij(rows[ELASTIC_ROW * (2 * j) + i], rows[ELASTIC_ROW * (2 * j + 1) + i], two_h);
    double mc = 0.0, md = 0.0;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            const double x = fabs(A[6 * i + j]), y = fabs(A[6 * i + j] - A[6 * j + i]);
            mc = x > mc ? x : mc, md = y > md ? y : md;
        }
    o->asym_C = mc > 0.0 ? md / mc : 0.0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) o->C[6 * i + j] = o->C[6 * j + i] = vib_mean(A[6 * i + j], A[6 * j + i]);
    const double* r0 = rows + ELASTIC_ROW * 12;
    for (int i = 0; i < 6; ++i) o->stress0[i] = r0[i] * ELASTIC_GPA;
    o->pressure = -(((r0[0] + r0[1]) + r0[2]) * ELASTIC_GPA) / 3.0;
    const bool has_S = ela_invert6(o->C, o->S, aug);
    ela_moduli(o->C, o->S, has_S, o->moduli);
    for (int i = 0; i < 36; ++i) A[i] = o->C[i];
    ela_eigvals6(A, ev, rot);
    int neg = 0;
    double lo = fabs(ev[0]), hi = lo;
    for (int k = 0; k < 6; ++k) {
        const double v = fabs(ev[k]);
        o->evals[k] = ev[k];
        neg += ev[k] < 0.0 ? 1 : 0;
        lo = v < lo ? v : lo, hi = v > hi ? v : hi;
    }
    o->cond = hi / lo;   // (inf when an eigenvalue is 0, NaN when all are: no threshold is applied here)
    o->n_negative = neg, o->n_unrelaxed = unrelaxed, o->status = has_S ? ELASTIC_OK : ELASTIC_SINGULAR;
}

}  // namespace mi
