// The per-item arithmetic of mi_sm_match (include/matinvent_hip_smatch.h), host and device: the metric of a lattice map, the
// mapped coordinates, the periodic cost of an atom pair, the species-constrained assignment and the RMS distance.  Conventions of
// sm_lattice.h: float64, every operation rounded separately, sqrt and floor the only library functions.
//
// An item is (map M, translation index j).  f2' = wrap(f2 M^-1); G = (L1 L1^T + (M L2)(M L2)^T) / 2; t = f1[first atom of the rarest
// species + j] - f2'[first atom of the rarest species]; the cost of (a, b) is the smallest (D + k)^T G (D + k) over k in {-1, 0, 1}^3 in
// lexicographic order (first minimum), D = (f2'[b] + t) - f1[a] with every component moved to [-1/2, 1/2) by D - floor(D + 1/2) (so a
// tie at +1/2 goes to -1/2).  Per species block the square assignment problem is solved by shortest augmenting paths: rows ascending, the
// next column the smallest tentative distance among the unscanned, ties to the lowest column.
#pragma once
#include "sm_lattice.h"

namespace mi {

#pragma clang fp contract(off)

// M L2 (rows) and the metric G [9] (symmetric, all nine written)
SM_HD void sm_metric(const double* L1, const double* L2, const int* M, double* G) {
    double ML[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) ML[3 * i + c] = ((double)M[3 * i] * L2[c] + (double)M[3 * i + 1] * L2[3 + c]) + (double)M[3 * i + 2] * L2[6 + c];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) G[3 * i + j] = (sm_dot3(L1 + 3 * i, L1 + 3 * j) + sm_dot3(ML + 3 * i, ML + 3 * j)) * 0.5;
}

// M^-1 as integers: adj(M) det(M), det(M) = +-1
SM_HD void sm_map_inverse(const int* M, int* Mi) {
    int A[9];
    sm_iadj3(M, A);
    const int d = sm_idet3(M);
#pragma unroll
    for (int i = 0; i < 9; ++i) Mi[i] = A[i] * d;
}

// f2' = wrap(f2 M^-1) of one atom
SM_HD void sm_map_frac(const double* f2, const int* Mi, double* out) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = sm_wrap01((f2[0] * (double)Mi[c] + f2[1] * (double)Mi[3 + c]) + f2[2] * (double)Mi[6 + c]);
}

SM_HD double sm_quad(const double* G, double x, double y, double z) {
    const double g0 = (G[0] * x + G[1] * y) + G[2] * z;
    const double g1 = (G[3] * x + G[4] * y) + G[5] * z;
    const double g2 = (G[6] * x + G[7] * y) + G[8] * z;
    return (x * g0 + y * g1) + z * g2;
}

// the cost d^2 of the pair (f1a, f2b' + t) and its vector u = D + k
SM_HD double sm_pair_cost(const double* G, const double* f1a, const double* f2b, const double* t, double* u) {
    double D[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double d = (f2b[c] + t[c]) - f1a[c];
        D[c] = d - floor(d + 0.5);
    }
    double best = sm_inf();
    u[0] = D[0], u[1] = D[1], u[2] = D[2];
#pragma unroll
    for (int kx = -1; kx <= 1; ++kx)
#pragma unroll
        for (int ky = -1; ky <= 1; ++ky)
#pragma unroll
            for (int kz = -1; kz <= 1; ++kz) {
                const double x = D[0] + (double)kx, y = D[1] + (double)ky, z = D[2] + (double)kz;
                const double q = sm_quad(G, x, y, z);
                if (q < best) best = q, u[0] = x, u[1] = y, u[2] = z;
            }
    return best;
}

// the tentative distance of column j through row i
SM_HD double sm_reduced(double min_val, double cost, double ui, double vj) { return ((min_val + cost) - ui) - vj; }

// The assignment of one square block in plain loops: cost [nb][nb] row-major, col4row out.  The kernel runs the same steps with a lane per
// column (struct_match.hip sm_wave_assign); work arrays of SM_MAX_ATOMS entries are the caller's.
struct SmAssignWork {
    double u[SM_MAX_ATOMS], v[SM_MAX_ATOMS], shortest[SM_MAX_ATOMS];
    int path[SM_MAX_ATOMS], row4col[SM_MAX_ATOMS];
    bool SR[SM_MAX_ATOMS], SC[SM_MAX_ATOMS];
};

inline bool sm_assign_serial(const double* cost, int nb, int* col4row, SmAssignWork* w) {
    for (int i = 0; i < nb; ++i) w->u[i] = 0.0, w->v[i] = 0.0, w->row4col[i] = -1, col4row[i] = -1, w->path[i] = -1;
    for (int cur = 0; cur < nb; ++cur) {
        for (int j = 0; j < nb; ++j) w->shortest[j] = sm_inf(), w->SR[j] = false, w->SC[j] = false;
        double min_val = 0.0;
        int i = cur, sink = -1;
        while (sink < 0) {
            w->SR[i] = true;
            double bv = sm_inf();
            int bj = 0x7fffffff;
            for (int j = 0; j < nb; ++j) {
                if (w->SC[j]) continue;
                const double r = sm_reduced(min_val, cost[(size_t)i * nb + j], w->u[i], w->v[j]);
                if (r < w->shortest[j]) w->shortest[j] = r, w->path[j] = i;
                if (sm_better(w->shortest[j], j, bv, bj)) bv = w->shortest[j], bj = j;
            }
            if (bj >= nb || !(bv < sm_inf())) return false;   // no column within reach: a cost that is not a finite number
            min_val = bv;
            w->SC[bj] = true;
            if (w->row4col[bj] < 0) sink = bj;
            else i = w->row4col[bj];
        }
        w->u[cur] = w->u[cur] + min_val;
        for (int r = 0; r < nb; ++r)
            if (w->SR[r] && r != cur) w->u[r] = w->u[r] + (min_val - w->shortest[col4row[r]]);
        for (int j = 0; j < nb; ++j)
            if (w->SC[j]) w->v[j] = w->v[j] - (min_val - w->shortest[j]);
        int j = sink;
        while (true) {
            const int r = w->path[j];
            w->row4col[j] = r;
            const int old = col4row[r];
            col4row[r] = j;
            j = old;
            if (r == cur) break;
        }
    }
    return true;
}

// mean of n vectors [n][3], a serial sum in ascending a, then / n
SM_HD void sm_mean(const double* u, int n, double* mean) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int a = 0; a < n; ++a) s0 = s0 + u[3 * a], s1 = s1 + u[3 * a + 1], s2 = s2 + u[3 * a + 2];
    mean[0] = s0 / (double)n, mean[1] = s1 / (double)n, mean[2] = s2 / (double)n;
}

// (u_a - mean)^T G (u_a - mean)
SM_HD double sm_centred(const double* G, const double* ua, const double* mean) { return sm_quad(G, ua[0] - mean[0], ua[1] - mean[1], ua[2] - mean[2]); }

// rms and max_dist from the n squared distances: a serial sum in ascending a
SM_HD void sm_rms(const double* d2, int n, double* rms, double* max_dist) {
    double s = 0.0, m = 0.0;
    for (int a = 0; a < n; ++a) {
        s = s + d2[a];
        m = d2[a] > m ? d2[a] : m;
    }
    const double ms = s / (double)n;   // (a quadratic form can round below zero: clamped)
    *rms = sqrt(ms > 0.0 ? ms : 0.0), *max_dist = sqrt(m);
}

}  // namespace mi
