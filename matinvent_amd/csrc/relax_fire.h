// The arithmetic of mi_relax_step (include/matinvent_hip_relax.h), host and device: one FIRE step of one crystal on the forces of
// a learned energy.  relax.hip's kernel calls these functions, and scripts/relax_host_check.cpp runs the same text against a plain loop
// under the host sanitizers.  Separately rounded fp32 operations: no contraction into FMAs.
//
// Conventions: lattice rows are cell vectors, cart = frac L.  So dE / dr_i = g_frac[i] L^-T and d frac = dr L^-1.  The degrees of freedom of
// a crystal of n atoms are R = n (+ 3 with relax_cell) ROWS of three: the atoms, then the cell's rows.  Every sum over the rows -- F.v,
// |v|^2, |F|^2, |dr|^2 -- is the per-row value ((a0 b0 + a1 b1) + a2 b2) reduced by ONE tree that is a function of R alone:
// for s = half(R), half(R) / 2, ..., 1:  a[i] += a[i + s] for every i < s with i + s < R   (half(R): half the smallest power of two >= R).
#pragma once
#include "guide_shift.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RELAX_HD __host__ __device__ inline
#else
#define RELAX_HD inline
#endif

namespace mi {

enum { RELAX_ACTIVE = 0, RELAX_CONVERGED = 1, RELAX_FAILED = 2, RELAX_EXHAUSTED = 3 };
// the per-crystal state: a float block and an int block
enum { RELAX_F_DT = 0, RELAX_F_ALPHA = 1, RELAX_F_E_FIRST = 2, RELAX_F_E_LAST = 3, RELAX_F_FMAX = 4, RELAX_F_DR = 5, RELAX_NF = 6 };
enum { RELAX_I_STATUS = 0, RELAX_I_NPOS = 1, RELAX_I_STEPS = 2, RELAX_NI = 3 };

struct RelaxParams {
    float dt, dt_max, maxstep, f_inc, f_dec, a_start, f_a, fmax;
    float scale;         // std[p] of the property's normaliser: the network's output is in normalised units
    float cell_factor;   // c_b; <= 0: the crystal's atom count
    float det_min;       // |det L| below it: FAILED
    int n_min, relax_cell, per_atom;
};

#pragma clang fp contract(off)

RELAX_HD float relax_dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

RELAX_HD int relax_rows(int n, int relax_cell) { return relax_cell ? n + 3 : n; }

// the first stride of the rows' tree
RELAX_HD int relax_tree_half(int R) {
    int p = 1;
    while (p < R) p <<= 1;
    return p >> 1;
}

RELAX_HD float relax_force_scale(const RelaxParams& p, int n) { return p.per_atom ? p.scale * (float)n : p.scale; }   // s_b
RELAX_HD float relax_cell_factor(const RelaxParams& p, int n) { return p.cell_factor > 0.0f ? p.cell_factor : (float)n; }   // c_b

RELAX_HD float relax_det3(const float* L) {
    const float c0 = L[4] * L[8] - L[5] * L[7], c1 = L[5] * L[6] - L[3] * L[8], c2 = L[3] * L[7] - L[4] * L[6];
    return (L[0] * c0 + L[1] * c1) + L[2] * c2;
}

// Li = L^-1 by cofactors, every element divided by det
RELAX_HD void relax_inv3(const float* L, float det, float* Li) {
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

// row r of the forces: an atom's F = -s g L^-T (F[k] = -s sum_d g[d] Li[k][d]), or a cell row's F = -s g_lat / c
RELAX_HD void relax_force_atom(const float* g, const float* Li, float s, float* F) {
    for (int k = 0; k < 3; ++k) F[k] = -(s * relax_dot3(g, Li + 3 * k));
}
RELAX_HD void relax_force_cell(const float* gl, float s, float c, float* F) {
    for (int k = 0; k < 3; ++k) F[k] = -(s * gl[k]) / c;
}

// what the sign of P = F.v decides, from the three sums
struct RelaxDecision {
    float dt, alpha, c1, c2;   // v = c1 v + c2 F (positive power) or 0, then v += dt F
    int npos, positive;
};
RELAX_HD RelaxDecision relax_decide(float P, float vv, float ff, float dt, float alpha, int npos, const RelaxParams& p) {
    RelaxDecision d;
    if (P > 0.0f) {
        d.positive = 1;
        d.c1 = 1.0f - alpha;
        d.c2 = alpha * (sqrtf(vv) / sqrtf(ff));
        if (npos > p.n_min) {
            const float g = dt * p.f_inc;
            dt = g < p.dt_max ? g : p.dt_max;
            alpha = alpha * p.f_a;
        }
        d.npos = npos + 1;
    } else {
        d.positive = 0;
        d.c1 = 0.0f;
        d.c2 = 0.0f;
        alpha = p.a_start;
        dt = dt * p.f_dec;
        d.npos = 0;
    }
    d.dt = dt;
    d.alpha = alpha;
    return d;
}

// one component of the velocity, then of the displacement dt v
RELAX_HD float relax_velocity(float v, float F, const RelaxDecision& d) {
    const float m = d.positive ? d.c1 * v + d.c2 * F : 0.0f;
    return m + d.dt * F;
}

// the factor of the norm clamp (1: no clamp)
RELAX_HD float relax_clamp(float norm, float maxstep) { return norm > maxstep ? maxstep / norm : 1.0f; }

// frac = pymod1(frac + dr L^-1)
RELAX_HD void relax_move_atom(float* x, const float* dr, const float* Li) {
    for (int d = 0; d < 3; ++d) x[d] = guide_mod1(x[d] + ((dr[0] * Li[d] + dr[1] * Li[3 + d]) + dr[2] * Li[6 + d]));
}

// the tree, serially (the kernel runs every level's additions side by side)
inline float relax_tree_sum_host(float* a, int R) {
    for (int s = relax_tree_half(R); s > 0; s >>= 1)
        for (int i = 0; i < s; ++i)
            if (i + s < R) a[i] += a[i + s];
    return a[0];
}

// One crystal, serially (the host check's form; the kernel distributes the same element functions over a workgroup): n atoms, the
// crystal's rows of every array; out_p = out[b][p]; work: 4 R floats.  Returns the status.
inline int relax_step_crystal_host(int n, const RelaxParams& p, float* frac, float* lat, float* vel_x, float* vel_l, float* fs, int* is,
                                   const float* g_frac, const float* g_lat, float out_p, float* work) {
    if (is[RELAX_I_STATUS] != RELAX_ACTIVE) return is[RELAX_I_STATUS];
    const int R = relax_rows(n, p.relax_cell);
    bool ok = guide_finite(out_p);
    for (int q = 0; q < 9; ++q) ok = ok && guide_finite(g_lat[q]) && guide_finite(lat[q]);
    for (int i = 0; i < 3 * n; ++i) ok = ok && guide_finite(g_frac[i]);
    const float det = relax_det3(lat);
    if (!ok || !(fabsf(det) >= p.det_min)) return is[RELAX_I_STATUS] = RELAX_FAILED;
    float Li[9];
    relax_inv3(lat, det, Li);
    const float s = relax_force_scale(p, n), c = relax_cell_factor(p, n);
    float* F = work;   // [R][3]
    float* red = work + 3 * (size_t)R;   // [R]
    float fm2 = 0.0f;
    for (int r = 0; r < R; ++r) {
        if (r < n) relax_force_atom(g_frac + 3 * r, Li, s, F + 3 * r);
        else relax_force_cell(g_lat + 3 * (r - n), s, c, F + 3 * r);
        const float n2 = relax_dot3(F + 3 * r, F + 3 * r);
        fm2 = n2 > fm2 ? n2 : fm2;
    }
    const float fm = sqrtf(fm2);
    if (is[RELAX_I_STEPS] == 0) fs[RELAX_F_E_FIRST] = out_p;
    fs[RELAX_F_E_LAST] = out_p;
    fs[RELAX_F_FMAX] = fm;
    if (fm < p.fmax) return is[RELAX_I_STATUS] = RELAX_CONVERGED;
    auto vrow = [&](int r) { return r < n ? vel_x + 3 * r : vel_l + 3 * (r - n); };
    for (int r = 0; r < R; ++r) red[r] = relax_dot3(F + 3 * r, vrow(r));
    const float P = relax_tree_sum_host(red, R);
    for (int r = 0; r < R; ++r) red[r] = relax_dot3(vrow(r), vrow(r));
    const float vv = relax_tree_sum_host(red, R);
    for (int r = 0; r < R; ++r) red[r] = relax_dot3(F + 3 * r, F + 3 * r);
    const float ff = relax_tree_sum_host(red, R);
    const RelaxDecision d = relax_decide(P, vv, ff, fs[RELAX_F_DT], fs[RELAX_F_ALPHA], is[RELAX_I_NPOS], p);
    for (int r = 0; r < R; ++r) {
        float* v = vrow(r);
        for (int k = 0; k < 3; ++k) {
            v[k] = relax_velocity(v[k], F[3 * r + k], d);
            F[3 * r + k] = d.dt * v[k];   // (the displacement takes the force's place)
        }
        red[r] = relax_dot3(F + 3 * r, F + 3 * r);
    }
    const float nd = sqrtf(relax_tree_sum_host(red, R));
    const float k = relax_clamp(nd, p.maxstep);
    for (int r = 0; r < R; ++r) {
        const float dr[3] = {F[3 * r] * k, F[3 * r + 1] * k, F[3 * r + 2] * k};
        if (r < n) relax_move_atom(frac + 3 * r, dr, Li);
        else
            for (int q = 0; q < 3; ++q) lat[3 * (r - n) + q] = lat[3 * (r - n) + q] + dr[q] / c;
    }
    fs[RELAX_F_DT] = d.dt;
    fs[RELAX_F_ALPHA] = d.alpha;
    fs[RELAX_F_DR] = nd;
    is[RELAX_I_NPOS] = d.npos;
    is[RELAX_I_STEPS] += 1;
    return RELAX_ACTIVE;
}

}  // namespace mi
