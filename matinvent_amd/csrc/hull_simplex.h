// The arithmetic of mi_hull_above (include/matinvent_hip_hull.h), host and device: the energy of a composition above the lower
// convex hull of a list of candidate phases, by a revised simplex from the elemental vertex.  hull.hip's two kernels call these functions
// with their thread index, and scripts/hull_host_check.cpp runs the same text with the thread index as a loop variable under the host
// sanitizers.  Everything is float64 and every product and addition is rounded separately (no contraction into FMAs), so that the numpy
// restatement tests/hull_ref64.py reproduces the bits.
//
// The problem of one query with d elements, fractions c[d] and candidates (x_i[d], E_i):  e_hull = min sum_i l_i E_i  subject to
// sum_i l_i x_i = c, l >= 0.  Start: the basis holds, per element k, the pure candidate (x_ik == 1) of lowest finite energy (ties: the
// lowest position); B^-1 = I, l = c.  Iterate: y = E_B B^-1; r_i = E_i - sum_k y_k x_ik over the non-basic candidates of finite energy;
// the smallest r_i enters (ties: the lowest position) unless it is >= -HULL_EPS (OK); u = B^-1 x_j; the smallest l_k / u_k over u_k >
// HULL_EPS leaves (ties: the lowest k; none: UNBOUNDED); l and B^-1 are updated in product form, l clamped at 0 from below.  After
// HULL_MAX_ITERS pivots without reaching the optimum: ITER_CAP.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HULL_HD __host__ __device__ inline
#else
#define HULL_HD inline
#endif

namespace mi {

enum { HULL_MAX_ELEMS = 8, HULL_MAX_ITERS = 256, HULL_THREADS = 256, HULL_COLS = HULL_MAX_ELEMS + 1 };
enum { HULL_OK = 0, HULL_NO_TERMINAL = 1, HULL_UNBOUNDED = 2, HULL_ITER_CAP = 3, HULL_BAD_QUERY = 4 };
enum { HULL_FLAG_SKIPPED = 1 };
enum { HULL_NO_POS = 0x7fffffff };
#define HULL_EPS 1e-12        /* the optimality threshold on a reduced cost and the pivot threshold on a direction component */
#define HULL_LDS_DOUBLES 4096 /* the LDS budget of a group's block: 32 KiB */

#pragma clang fp contract(off)

HULL_HD bool hull_finite(double v) { return v - v == 0.0; }
HULL_HD double hull_nan() { return (double)__builtin_nanf(""); }
HULL_HD double hull_inf() { return (double)__builtin_inff(); }

// the order of the argmin: the smaller value, and of equal values the lower position -- exact, so any tree gives the same pair
HULL_HD bool hull_better(double v, int p, double ov, int op) { return v < ov || (v == ov && p < op); }

// ---- the views ----------------------------------------------------------------------------------------------------------------------------
struct HullBank {
    const int* nelem;       // [M]
    const int* Z;           // [M][8], sorted ascending over the first nelem
    const double* frac;     // [M][8]
    const double* energy;   // [M], per atom; NaN allowed
    int M;
};

// A group's staged block: column k (k < d) of the fractions at x + k * nc, the energies at x + d * nc, the bank rows at row (-1: skipped).
struct HullBlock {
    const double* x;
    const int* row;
    int nc, d;
};

HULL_HD double hull_block_frac(const HullBlock& b, int i, int k) { return b.x[(size_t)k * (size_t)b.nc + (size_t)i]; }
HULL_HD double hull_block_energy(const HullBlock& b, int i) { return b.x[(size_t)b.d * (size_t)b.nc + (size_t)i]; }

// ---- staging: one candidate of one group ----------------------------------------------------------------------------------------------------
// Writes position i of the block (fractions in the group's element order, the energy, the bank row).  Returns 1 when the guard skipped the
// candidate (an index outside the bank, n_elem outside 1 .. 8, an element outside the group's set, a fraction that is not finite): its
// energy is NaN, its fractions 0, its row -1, and nothing was read through the index.
HULL_HD int hull_stage_candidate(const HullBank& bank, const int* gZ, int d, int idx, double* x, int* row, int nc, int i) {
    double f[HULL_MAX_ELEMS];
#pragma unroll
    for (int k = 0; k < HULL_MAX_ELEMS; ++k) f[k] = 0.0;
    bool ok = idx >= 0 && idx < bank.M;
    double e = hull_nan();
    if (ok) {
        const int n = bank.nelem[idx];
        ok = n >= 1 && n <= HULL_MAX_ELEMS;
        if (ok) {
            for (int a = 0; a < n; ++a) {
                const int z = bank.Z[(size_t)idx * HULL_MAX_ELEMS + a];
                const double v = bank.frac[(size_t)idx * HULL_MAX_ELEMS + a];
                bool found = false;
#pragma unroll
                for (int k = 0; k < HULL_MAX_ELEMS; ++k)
                    if (k < d && gZ[k] == z && !found) {
                        f[k] = v;
                        found = true;
                    }
                ok = ok && found && hull_finite(v);
            }
            if (ok) e = bank.energy[idx];
        }
    }
#pragma unroll
    for (int k = 0; k < HULL_MAX_ELEMS; ++k)
        if (k < d) x[(size_t)k * (size_t)nc + (size_t)i] = ok ? f[k] : 0.0;
    x[(size_t)d * (size_t)nc + (size_t)i] = e;
    row[i] = ok ? idx : -1;
    return ok ? 0 : 1;
}

// a group's element list: 1 .. 8 strictly ascending atomic numbers
HULL_HD bool hull_group_ok(const int* gZ, int d) {
    if (d < 1 || d > HULL_MAX_ELEMS) return false;
    for (int k = 1; k < d; ++k)
        if (!(gZ[k] > gZ[k - 1])) return false;
    return true;
}

// ---- the d x d state of one query (one lane owns it; in LDS on the device) ----------------------------------------------------------------
struct HullState {
    double Binv[HULL_MAX_ELEMS * HULL_MAX_ELEMS];   // row-major
    double c[HULL_MAX_ELEMS], lam[HULL_MAX_ELEMS], EB[HULL_MAX_ELEMS], y[HULL_MAX_ELEMS], u[HULL_MAX_ELEMS], xj[HULL_MAX_ELEMS];
    int basis[HULL_MAX_ELEMS];                      // candidate positions
    int d, iters, status, done;
};

// y = E_B B^-1: y_k = sum_j E_B[j] B^-1[j][k], j ascending from 0.0
HULL_HD void hull_duals(HullState& s) {
    for (int k = 0; k < s.d; ++k) {
        double a = 0.0;
        for (int j = 0; j < s.d; ++j) a = a + s.EB[j] * s.Binv[j * HULL_MAX_ELEMS + k];
        s.y[k] = a;
    }
}

// Start from the elemental vertex.  On entry s.c holds the query's fractions, s.basis[k] the position of element k's terminal (HULL_NO_POS:
// none) and s.EB[k] its energy.
HULL_HD void hull_start(HullState& s, int d) {
    s.d = d, s.iters = 0, s.status = HULL_OK, s.done = 0;
    bool bad = false;
    for (int k = 0; k < d; ++k) bad = bad || !(hull_finite(s.c[k]) && s.c[k] >= 0.0);
    if (bad) {
        s.status = HULL_BAD_QUERY, s.done = 1;
        return;
    }
    for (int k = 0; k < d; ++k) {
        if (s.basis[k] == HULL_NO_POS) s.status = HULL_NO_TERMINAL, s.done = 1;
        for (int j = 0; j < d; ++j) s.Binv[k * HULL_MAX_ELEMS + j] = k == j ? 1.0 : 0.0;
        s.lam[k] = s.c[k];
    }
    if (!s.done) hull_duals(s);
}

// e_hull = sum_k y_k c_k, k ascending from 0.0
HULL_HD double hull_value(const HullState& s) {
    double a = 0.0;
    for (int k = 0; k < s.d; ++k) a = a + s.y[k] * s.c[k];
    return a;
}

HULL_HD bool hull_in_basis(const int* basis, int d, int i) {
    bool in = false;
#pragma unroll
    for (int k = 0; k < HULL_MAX_ELEMS; ++k) in = in || (k < d && basis[k] == i);
    return in;
}

// r_i = E_i - sum_k y_k x_ik of position i of the block: a function of the row and y alone
HULL_HD double hull_reduced_cost(const HullBlock& b, int i, const double* y) {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < HULL_MAX_ELEMS; ++k)
        if (k < b.d) a = a + y[k] * hull_block_frac(b, i, k);
    return hull_block_energy(b, i) - a;
}

// thread tid of T: the best terminal of element k among its positions tid, tid + T, ...
HULL_HD void hull_terminal_thread(const HullBlock& b, int k, int tid, int T, double& best, int& pos) {
    best = hull_inf(), pos = HULL_NO_POS;
    for (int i = tid; i < b.nc; i += T) {
        const double e = hull_block_energy(b, i);
        if (hull_block_frac(b, i, k) == 1.0 && hull_finite(e) && hull_better(e, i, best, pos)) best = e, pos = i;
    }
}

// thread tid of T: the smallest reduced cost among its positions tid, tid + T, ... that are non-basic and of finite energy
HULL_HD void hull_price_thread(const HullBlock& b, const double* y, const int* basis, int tid, int T, double& best, int& pos) {
    best = hull_inf(), pos = HULL_NO_POS;
    for (int i = tid; i < b.nc; i += T) {
        if (!hull_finite(hull_block_energy(b, i)) || hull_in_basis(basis, b.d, i)) continue;
        const double r = hull_reduced_cost(b, i, y);
        if (hull_better(r, i, best, pos)) best = r, pos = i;
    }
}

// One decision of the owning lane after pricing found (rmin, j): stop at the optimum or the cap, else pivot candidate j (fractions in s.xj,
// energy Ej) into the basis and recompute the duals.  Sets s.done when the query is finished.
HULL_HD void hull_decide(HullState& s, double rmin, int j, double Ej) {
    if (j == HULL_NO_POS || rmin >= -HULL_EPS) {
        s.done = 1;
        return;
    }
    if (s.iters >= HULL_MAX_ITERS) {
        s.status = HULL_ITER_CAP, s.done = 1;
        return;
    }
    const int d = s.d;
    for (int k = 0; k < d; ++k) {
        double a = 0.0;
        for (int q = 0; q < d; ++q) a = a + s.Binv[k * HULL_MAX_ELEMS + q] * s.xj[q];
        s.u[k] = a;
    }
    int r = -1;
    double theta = hull_inf();
    for (int k = 0; k < d; ++k)
        if (s.u[k] > HULL_EPS) {
            const double t = s.lam[k] / s.u[k];
            if (t < theta) theta = t, r = k;
        }
    if (r < 0) {
        s.status = HULL_UNBOUNDED, s.done = 1;
        return;
    }
    const double ur = s.u[r];
    for (int q = 0; q < d; ++q) s.Binv[r * HULL_MAX_ELEMS + q] = s.Binv[r * HULL_MAX_ELEMS + q] / ur;
    for (int k = 0; k < d; ++k) {
        if (k == r) continue;
        const double uk = s.u[k];
        for (int q = 0; q < d; ++q) s.Binv[k * HULL_MAX_ELEMS + q] = s.Binv[k * HULL_MAX_ELEMS + q] - uk * s.Binv[r * HULL_MAX_ELEMS + q];
        const double l = s.lam[k] - theta * uk;
        s.lam[k] = l > 0.0 ? l : 0.0;
    }
    s.lam[r] = theta;
    s.EB[r] = Ej;
    s.basis[r] = j;
    s.iters += 1;
    hull_duals(s);
}

}  // namespace mi
