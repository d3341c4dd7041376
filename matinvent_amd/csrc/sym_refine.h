// The arithmetic of the refined structure (include/matinvent_hip_sym_refine.h), host and device: the site maps of the operations
// mi_sym_find returned, their best-fit translations, the projection of the coordinates and of the metric onto the group, the site orbits
// and the Cholesky cell.  sym_refine.hip calls these functions with its thread index, scripts/sym_refine_host_check.cpp runs the same text
// with the index as a loop variable under the host sanitizers.  Conventions of sym_ops.h, whose nearest site, 27-image pair cost, wrap and
// rigid metric are used as they stand: float64 or exact integers, every operation rounded separately, sqrt and floor the only library
// functions, so that tests/refine_ref64.py reproduces the bits.
//
// Everything is in the reduced basis of the prepared set: an operation is g_k(f) = f W_k^-1 + t_k, W_k^-1 = adj(W_k) det(W_k) in integers.
// The site map sigma_k(i) is kept as one byte a site (at most 64 sites), row k at sig + 64 k.
#pragma once
#include "sym_ops.h"

namespace mi {

enum { SYM_REFINE_FAIL = 1024, REFINE_INFO = 8, REFINE_STAT = 4, REFINE_ROW = 64 };

#pragma clang fp contract(off)

// the species block [b0, b0 + nb) of site i
SM_HD void refine_block(const int* spec_off, int nspec, int i, int* b0, int* nb) {
    int s = 0;
    for (int e = 1; e < nspec; ++e) s += spec_off[e] <= i ? 1 : 0;
    *b0 = spec_off[s], *nb = spec_off[s + 1] - spec_off[s];
}

// the image wrap(x W^-1) of one site
SM_HD void refine_image(const double* x, const int* W, double* img) {
    int Mi[9];
    sm_map_inverse(W, Mi);
    sm_map_frac(x, Mi, img);
}

// sigma_k(i): the site of i's block nearest to g_k(x_i); d2: the squared length of the residual
SM_HD int refine_sigma(const double* G, const double* f, int b0, int nb, int i, const int* W, const double* t, double* d2) {
    double img[3], u[3];
    refine_image(f + 3 * i, W, img);
    return sym_nearest(G, f, b0, nb, img, t, u, d2);
}

SM_HD int refine_bits(uint64_t m) {
    int c = 0;
    for (; m; m &= m - 1) ++c;
    return c;
}

// sigma_k is a bijection of the n sites
SM_HD bool refine_bijection(const unsigned char* sig, int n) {
    uint64_t mask = 0;
    for (int i = 0; i < n; ++i) mask |= 1ull << sig[i];
    return refine_bits(mask) == n;
}

// the refined translation of operation k: t - (the sum of the residuals r_k(i) in ascending i) / n, the residual of (i, sigma_k(i)) being
// the pair cost's vector as sym_nearest formed it
SM_HD void refine_translation(const double* G, const double* f, int n, const unsigned char* sig, const int* W, const double* t, double* tbar) {
    int Mi[9];
    sm_map_inverse(W, Mi);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < n; ++i) {
        double img[3], u[3];
        sm_map_frac(f + 3 * i, Mi, img);
        sm_pair_cost(G, f + 3 * sig[i], img, t, u);
        s0 = s0 + u[0], s1 = s1 + u[1], s2 = s2 + u[2];
    }
    tbar[0] = t[0] - s0 / (double)n, tbar[1] = t[1] - s1 / (double)n, tbar[2] = t[2] - s2 / (double)n;
}

// W G W^T of an integer W: (W G) first, then (W G) W^T, every entry a sum of three products in ascending index
SM_HD void refine_congruence(const int* W, const double* G, double* out) {
    double A[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) A[3 * i + j] = ((double)W[3 * i] * G[j] + (double)W[3 * i + 1] * G[3 + j]) + (double)W[3 * i + 2] * G[6 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) out[3 * i + j] = (A[3 * i] * (double)W[3 * j] + A[3 * i + 1] * (double)W[3 * j + 1]) + A[3 * i + 2] * (double)W[3 * j + 2];
}

// The refined cell.  lat32: the caller's cell; rot: the nops rotation parts.  T: the transform of mi_sm_prepare, recomputed; Gbar: the mean
// of W G W^T over the operations in ascending k, G the metric of T x lat32; change: max |Gbar - G| / max |G|; out: the lower Cholesky
// factor of T^-1 Gbar T^-T as float32 (rows are the cell vectors: a along x, b in the xy plane).  false: a pivot that is not positive.
SM_HD bool refine_cell(const float* lat32, const int* rot, int nops, int* T, double* Gbar, double* change, float* out) {
    double L0[9], Lr[9], G[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) L0[e] = (double)lat32[e], Gbar[e] = 0.0;
    sm_reduce(L0, T, Lr);   // (the prepare status is OK: the reduction ended)
    sym_metric(Lr, G);
    for (int k = 0; k < nops; ++k) {
        double B[9];
        refine_congruence(rot + 9 * k, G, B);
#pragma unroll
        for (int e = 0; e < 9; ++e) Gbar[e] = Gbar[e] + B[e];
    }
    double dmax = 0.0, gmax = 0.0;
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        Gbar[e] = Gbar[e] / (double)nops;
        const double d = sm_abs(Gbar[e] - G[e]), g = sm_abs(G[e]);
        dmax = d > dmax ? d : dmax, gmax = g > gmax ? g : gmax;
    }
    *change = dmax / gmax;
    int Ti[9];
    double Gc[9];
    sm_iadj3(T, Ti);   // (det T = 1)
    refine_congruence(Ti, Gbar, Gc);
#pragma unroll
    for (int e = 0; e < 9; ++e) out[e] = 0.0f;
    if (!(Gc[0] > 0.0)) return false;
    const double l00 = sqrt(Gc[0]), l10 = Gc[3] / l00, l20 = Gc[6] / l00;
    const double p1 = Gc[4] - l10 * l10;
    if (!(p1 > 0.0)) return false;
    const double l11 = sqrt(p1), l21 = (Gc[7] - l20 * l10) / l11;
    const double p2 = (Gc[8] - l20 * l20) - l21 * l21;
    if (!(p2 > 0.0)) return false;
    out[0] = (float)l00, out[3] = (float)l10, out[4] = (float)l11, out[6] = (float)l20, out[7] = (float)l21, out[8] = (float)sqrt(p2);
    return true;
}

// Site i.  move: (the sum over k in ascending order of the minimum image of (x_sigma_k(i) - tbar_k) W_k - x_i) / nops; xbar = x_i + move;
// q: its squared length in G, clamped at 0; low: the lowest perm among the sites sigma_k(i); mult: their number; stab: #{k: sigma_k(i) = i}.
SM_HD void refine_site(const double* G, const double* f, int i, const unsigned char* sig, const int* rot, const double* tbar, int nops, const int* perm,
                       double* xbar, double* q, int* low, int* mult, int* stab) {
    const double zero[3] = {0.0, 0.0, 0.0};
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    uint64_t mask = 0;
    int st = 0, lo = 0x7fffffff;
    for (int k = 0; k < nops; ++k) {
        const int j = sig[REFINE_ROW * k + i];
        const int* W = rot + 9 * k;
        const double y0 = f[3 * j] - tbar[3 * k], y1 = f[3 * j + 1] - tbar[3 * k + 1], y2 = f[3 * j + 2] - tbar[3 * k + 2];
        double z[3], u[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) z[c] = (y0 * (double)W[c] + y1 * (double)W[3 + c]) + y2 * (double)W[6 + c];
        sm_pair_cost(G, f + 3 * i, z, zero, u);
        s0 = s0 + u[0], s1 = s1 + u[1], s2 = s2 + u[2];
        mask |= 1ull << j;
        st += j == i ? 1 : 0;
        lo = perm[j] < lo ? perm[j] : lo;
    }
    const double m0 = s0 / (double)nops, m1 = s1 / (double)nops, m2 = s2 / (double)nops;
    xbar[0] = f[3 * i] + m0, xbar[1] = f[3 * i + 1] + m1, xbar[2] = f[3 * i + 2] + m2;
    const double qq = sm_quad(G, m0, m1, m2);
    *q = qq > 0.0 ? qq : 0.0, *low = lo, *mult = refine_bits(mask), *stab = st;
}

// the refined coordinates of one site in the caller's basis as float32 in [0, 1): wrap(xbar T), sym_prim_frac's rounding rule
SM_HD void refine_frac(const double* xbar, const int* T, float* out) {
    double Td[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) Td[e] = (double)T[e];
    sym_prim_frac(xbar, Td, out);
}

// step s of the fixed tree over 64 slots: slot i < s takes slot i + s (s = 32, 16 .. 1)
SM_HD double refine_tree_add(double a, double b) { return a + b; }
SM_HD double refine_max(double a, double b) { return b > a ? b : a; }

// the statistics row from the tree's results: max move, rms move, the cell change, max residual
SM_HD void refine_stats(double qmax, double qsum, int n, double change, double d2max, double* row) {
    row[0] = sqrt(qmax), row[1] = sqrt(qsum / (double)n), row[2] = change, row[3] = sqrt(d2max);
}

}  // namespace mi
