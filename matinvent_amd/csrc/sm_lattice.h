// The lattice arithmetic of the structure matcher (include/matinvent_hip_smatch.h), host and device: the cell reduction and the
// per-atom sort of mi_sm_prepare, and the enumeration, length, angle and determinant tests of mi_sm_match's lattice maps.
// struct_match.hip calls these functions with its lane or thread index, scripts/struct_match_host_check.cpp runs the same text with the
// index as a loop variable under the host sanitizers.  Everything is float64 (or exact integers) and every product and addition is rounded
// separately (no contraction into FMAs); the only library functions are sqrt and floor, both exact, so that the restatement
// tests/sm_ref64.py reproduces the bits.
//
// Rows of a lattice are its cell vectors.  The reduction is a greedy Minkowski pair reduction on an integer transform T (reduced = T x
// given, det T = 1), tolerance-free: per sweep, row i in 0, 1, 2 first takes L_i - m L_j for j != i ascending, m the nearest integer of
// (L_i . L_j) / (L_j . L_j), when that is strictly shorter, then the strictly shortest of L_i + s L_j + t L_k over (s, t) in {-1, 0, 1}^2
// in lexicographic order (j < k the other two rows).  Rows are recomputed from T and the given cell after every accepted step, so nothing
// accumulates.  It ends at the first sweep without a change; SM_REDUCE_SWEEPS sweeps or an entry of T beyond SM_T_MAX: REDUCE_CAP.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SM_HD __host__ __device__ inline
#else
#define SM_HD inline
#endif

namespace mi {

enum { SM_MAX_ATOMS = 64, SM_MAX_SPECIES = 16, SM_MAX_Z = 118, SM_MAX_MAPS = 256, SM_MAX_CAND = 128, SM_BOX_CAP = 32768, SM_THREADS = 256 };
enum { SM_REDUCE_SWEEPS = 64, SM_T_MAX = 1 << 20, SM_ROOT_ITERS = 200 };
enum { SM_PREP_OK = 0, SM_PREP_BAD_INPUT = 1, SM_PREP_TOO_MANY_ATOMS = 2, SM_PREP_TOO_MANY_SPECIES = 3, SM_PREP_DEGENERATE_CELL = 4, SM_PREP_REDUCE_CAP = 5 };
enum { SM_OK = 0, SM_NO_LATTICE = 1, SM_BOX_CAP_HIT = 2, SM_MAP_CAP_HIT = 3, SM_SPECIES_MISMATCH = 4, SM_BAD_PAIR = 5, SM_NOT_PREPARED = 6 };
#define SM_MIN_VOLUME 0.1 /* A^3: below it the cell is DEGENERATE_CELL */

#pragma clang fp contract(off)

SM_HD bool sm_finite(double v) { return v - v == 0.0; }
SM_HD double sm_inf() { return (double)__builtin_inff(); }
SM_HD double sm_abs(double v) { return v < 0.0 ? -v : v; }

// the order of every argmin: the smaller value, and of equal values the lower index -- exact, so any tree gives the same pair
SM_HD bool sm_better(double v, int p, double ov, int op) { return v < ov || (v == ov && p < op); }

SM_HD double sm_dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

SM_HD double sm_det3(const double* L) {
    return (L[0] * (L[4] * L[8] - L[5] * L[7]) - L[1] * (L[3] * L[8] - L[5] * L[6])) + L[2] * (L[3] * L[7] - L[4] * L[6]);
}

// inv = L^-1 by cofactors over det (the caller has checked det)
SM_HD void sm_inv3(const double* L, double det, double* inv) {
    inv[0] = (L[4] * L[8] - L[5] * L[7]) / det;
    inv[1] = (L[2] * L[7] - L[1] * L[8]) / det;
    inv[2] = (L[1] * L[5] - L[2] * L[4]) / det;
    inv[3] = (L[5] * L[6] - L[3] * L[8]) / det;
    inv[4] = (L[0] * L[8] - L[2] * L[6]) / det;
    inv[5] = (L[2] * L[3] - L[0] * L[5]) / det;
    inv[6] = (L[3] * L[7] - L[4] * L[6]) / det;
    inv[7] = (L[1] * L[6] - L[0] * L[7]) / det;
    inv[8] = (L[0] * L[4] - L[1] * L[3]) / det;
}

SM_HD int sm_idet3(const int* M) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// adj(M) (the transposed cofactors): M^-1 = adj(M) * det(M) when det(M) = +-1
SM_HD void sm_iadj3(const int* M, int* A) {
    A[0] = M[4] * M[8] - M[5] * M[7];
    A[1] = M[2] * M[7] - M[1] * M[8];
    A[2] = M[1] * M[5] - M[2] * M[4];
    A[3] = M[5] * M[6] - M[3] * M[8];
    A[4] = M[0] * M[8] - M[2] * M[6];
    A[5] = M[2] * M[3] - M[0] * M[5];
    A[6] = M[3] * M[7] - M[4] * M[6];
    A[7] = M[1] * M[6] - M[0] * M[7];
    A[8] = M[0] * M[4] - M[1] * M[3];
}

// x with x^3 = r (r > 0, finite) by Newton from above, x <- (2 x + r / x^2) / 3 from max(r, 1), until it stops decreasing: sums, products
// and quotients only, so host and device agree (the library cube roots differ in their last bit)
SM_HD double sm_cuberoot(double r) {
    double x = r > 1.0 ? r : 1.0;
    for (int it = 0; it < SM_ROOT_ITERS; ++it) {
        const double nx = ((x + x) + r / (x * x)) / 3.0;
        if (!(nx < x)) break;
        x = nx;
    }
    return x;
}

// row i of T x L0
SM_HD void sm_trow(const int* T, const double* L0, int i, double* row) {
#pragma unroll
    for (int c = 0; c < 3; ++c) row[c] = ((double)T[3 * i] * L0[c] + (double)T[3 * i + 1] * L0[3 + c]) + (double)T[3 * i + 2] * L0[6 + c];
}

// The reduction.  L0: the given cell.  T, L: the transform and the reduced cell T x L0.  Returns false on REDUCE_CAP.
SM_HD bool sm_reduce(const double* L0, int* T, double* L) {
#pragma unroll
    for (int i = 0; i < 9; ++i) T[i] = (i % 4 == 0) ? 1 : 0, L[i] = L0[i];
    for (int sweep = 0; sweep < SM_REDUCE_SWEEPS; ++sweep) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {   // the pair step against j != i, ascending
                const int j = (jj == 0) ? (i == 0 ? 1 : 0) : (i == 2 ? 1 : 2);
                const double q = sm_dot3(L + 3 * i, L + 3 * j) / sm_dot3(L + 3 * j, L + 3 * j);
                const double m = floor(q + 0.5);
                if (m != 0.0 && sm_abs(m) <= (double)SM_T_MAX) {
                    int Tn[9];
#pragma unroll
                    for (int e = 0; e < 9; ++e) Tn[e] = T[e];
                    bool big = false;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double t = (double)T[3 * i + c] - m * (double)T[3 * j + c];
                        big = big || sm_abs(t) > (double)SM_T_MAX;
                        Tn[3 * i + c] = big ? 0 : (int)t;
                    }
                    if (big) return false;
                    double row[3];
                    sm_trow(Tn, L0, i, row);
                    if (sm_dot3(row, row) < sm_dot3(L + 3 * i, L + 3 * i)) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) T[3 * i + c] = Tn[3 * i + c], L[3 * i + c] = row[c];
                        changed = true;
                    }
                }
            }
            const int j = i == 0 ? 1 : 0, k = i == 2 ? 1 : 2;   // the combination step
            double best = sm_dot3(L + 3 * i, L + 3 * i);
            int bs = 0, bt = 0;
#pragma unroll
            for (int s = -1; s <= 1; ++s)
#pragma unroll
                for (int t = -1; t <= 1; ++t) {
                    if (s == 0 && t == 0) continue;
                    int Tn[9];
#pragma unroll
                    for (int e = 0; e < 9; ++e) Tn[e] = T[e];
#pragma unroll
                    for (int c = 0; c < 3; ++c) Tn[3 * i + c] = T[3 * i + c] + s * T[3 * j + c] + t * T[3 * k + c];
                    double row[3];
                    sm_trow(Tn, L0, i, row);
                    const double l2 = sm_dot3(row, row);
                    if (l2 < best) best = l2, bs = s, bt = t;
                }
            if (bs != 0 || bt != 0) {
                bool big = false;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    T[3 * i + c] = T[3 * i + c] + bs * T[3 * j + c] + bt * T[3 * k + c];
                    big = big || T[3 * i + c] > SM_T_MAX || T[3 * i + c] < -SM_T_MAX;
                }
                if (big) return false;
                double row[3];
                sm_trow(T, L0, i, row);
#pragma unroll
                for (int c = 0; c < 3; ++c) L[3 * i + c] = row[c];
                changed = true;
            }
        }
        if (!changed) return true;
    }
    return false;
}

// x - floor(x) in [0, 1): a result that rounds to 1 is 0
SM_HD double sm_wrap01(double x) {
    const double w = x - floor(x);
    return w >= 1.0 ? 0.0 : w;
}

// ---- mi_sm_prepare: the cell of one crystal ---------------------------------------------------------------------------------------------------
// lat32: the given cell [9] (every entry finite: the caller checked).  Outputs: T, the reduced cell scaled to unit volume per atom, its
// inverse.  Returns the status (OK, DEGENERATE_CELL, REDUCE_CAP); on a failure the outputs are not meaningful.
SM_HD int sm_prepare_cell(const float* lat32, int n, int* T, double* Ls, double* inv) {
    double L0[9], L[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) L0[i] = (double)lat32[i];
    const double vol0 = sm_abs(sm_det3(L0));
    if (!(vol0 >= SM_MIN_VOLUME)) return SM_PREP_DEGENERATE_CELL;
    if (!sm_reduce(L0, T, L)) return SM_PREP_REDUCE_CAP;
    const double vol = sm_abs(sm_det3(L));   // (det T = 1: the given cell's volume up to rounding)
    const double s = sm_cuberoot((double)n / vol);
#pragma unroll
    for (int i = 0; i < 9; ++i) Ls[i] = L[i] * s;
    sm_inv3(Ls, sm_det3(Ls), inv);
    return SM_PREP_OK;
}

// ---- mi_sm_prepare: one atom (lane a) of one crystal ------------------------------------------------------------------------------------------
// types: the crystal's n atomic numbers, each in 1 .. SM_MAX_Z (the caller checked).  rank: a's place in the stable ascending sort.  first:
// a is the first atom of its species.  sidx: the number of species below a's.  cnt: the atoms of a's species.
SM_HD void sm_sort_lane(const int* types, int n, int a, int* rank, bool* first, int* sidx, int* cnt) {
    const int za = types[a];
    int r = 0, s = 0, c = 0;
    bool f = true;
    for (int b = 0; b < n; ++b) {
        const int zb = types[b];
        r += (zb < za || (zb == za && b < a)) ? 1 : 0;
        c += zb == za ? 1 : 0;
        f = f && !(zb == za && b < a);
        if (zb < za) {   // b counts when it is the first of its species
            bool fb = true;
            for (int e = 0; e < b; ++e) fb = fb && types[e] != zb;
            s += fb ? 1 : 0;
        }
    }
    *rank = r, *first = f, *sidx = s, *cnt = c;
}

// the coordinates of one atom in the reduced basis: wrap(f T^-1), T^-1 = adj(T) (det T = 1)
SM_HD void sm_reduced_frac(const float* f32, const int* T, double* out) {
    int A[9];
    sm_iadj3(T, A);
    const double f0 = (double)f32[0], f1 = (double)f32[1], f2 = (double)f32[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = sm_wrap01((f0 * (double)A[c] + f1 * (double)A[3 + c]) + f2 * (double)A[6 + c]);
}

// the rarest species of a block table: fewest atoms, ties to the lowest atomic number (the table ascends in Z, so the first minimum)
SM_HD int sm_rarest(const int* spec_off, int nspec) {
    int best = 0;
    for (int s = 1; s < nspec; ++s)
        if (spec_off[s + 1] - spec_off[s] < spec_off[best + 1] - spec_off[best]) best = s;
    return best;
}

// ---- mi_sm_match: the lattice maps ------------------------------------------------------------------------------------------------------------
struct SmTarget {
    double len[3];   // |a1|, |b1|, |c1|
    double ct[3];    // clamped cosines of (b, c), (a, c), (a, b)
    double maxlen;
};

SM_HD double sm_clamp1(double c) { return c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c); }

SM_HD double sm_cos(const double* u, double lu, const double* v, double lv) { return sm_clamp1(sm_dot3(u, v) / (lu * lv)); }

SM_HD void sm_target(const double* L1, SmTarget* t) {
#pragma unroll
    for (int i = 0; i < 3; ++i) t->len[i] = sqrt(sm_dot3(L1 + 3 * i, L1 + 3 * i));
    t->maxlen = t->len[0] > t->len[1] ? t->len[0] : t->len[1];
    t->maxlen = t->maxlen > t->len[2] ? t->maxlen : t->len[2];
    t->ct[0] = sm_cos(L1 + 3, t->len[1], L1 + 6, t->len[2]);
    t->ct[1] = sm_cos(L1, t->len[0], L1 + 6, t->len[2]);
    t->ct[2] = sm_cos(L1, t->len[0], L1 + 3, t->len[1]);
}

// the enumeration box |k_i| <= bound[i] = floor((1 + ltol) maxlen |b2_i*|), b2_i* column i of inv2; returns the number of points, or -1
// when it exceeds SM_BOX_CAP
SM_HD int sm_box(const SmTarget& t, const double* inv2, double ltol, int* bound) {
    int64_t pts = 1;
    bool over = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double bl = sqrt((inv2[i] * inv2[i] + inv2[3 + i] * inv2[3 + i]) + inv2[6 + i] * inv2[6 + i]);
        const double b = floor(((1.0 + ltol) * t.maxlen) * bl);
        over = over || !(b <= (double)SM_BOX_CAP);
        bound[i] = over ? 0 : (int)b;
        pts *= (int64_t)(2 * bound[i] + 1);
        over = over || pts > SM_BOX_CAP;
    }
    return over ? -1 : (int)pts;
}

// point p of the box in lexicographic order: k, v = k L2, |v|
SM_HD void sm_box_point(int p, const int* bound, const double* L2, int* k, double* v, double* len) {
    const int n1 = 2 * bound[1] + 1, n2 = 2 * bound[2] + 1;
    k[0] = p / (n1 * n2) - bound[0], k[1] = (p / n2) % n1 - bound[1], k[2] = p % n2 - bound[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = ((double)k[0] * L2[c] + (double)k[1] * L2[3 + c]) + (double)k[2] * L2[6 + c];
    *len = sqrt(sm_dot3(v, v));
}

SM_HD bool sm_length_ok(double len, double target, double ltol) { return sm_abs(len / target - 1.0) <= ltol; }

// the angle between two directions of cosine c is within the tolerance of the target's (cosine ct): cos(difference) >= cos_tol
SM_HD bool sm_angle_ok(double c, double ct, double cos_tol) { return c * ct + sqrt(1.0 - c * c) * sqrt(1.0 - ct * ct) >= cos_tol; }

// one triple of candidates (vectors vi, vj, vk with lengths and integer rows): the three angles, then |det| = 1
SM_HD bool sm_triple_ok(const SmTarget& t, const double* vi, double li, const int* ki, const double* vj, double lj, const int* kj, const double* vk,
                        double lk, const int* kk, double cos_tol) {
    if (!sm_angle_ok(sm_cos(vi, li, vj, lj), t.ct[2], cos_tol)) return false;
    if (!sm_angle_ok(sm_cos(vi, li, vk, lk), t.ct[1], cos_tol)) return false;
    if (!sm_angle_ok(sm_cos(vj, lj, vk, lk), t.ct[0], cos_tol)) return false;
    const int M[9] = {ki[0], ki[1], ki[2], kj[0], kj[1], kj[2], kk[0], kk[1], kk[2]};
    const int d = sm_idet3(M);
    return d == 1 || d == -1;
}

}  // namespace mi
