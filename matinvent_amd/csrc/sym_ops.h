// The arithmetic of the symmetry finder (include/matinvent_hip_sym.h), host and device: the length rule and the box of the
// self-maps of a reduced cell, the nearest atom of an image, the class of a rotation part, the point-group table and the triple test of
// the primitive cell.  symmetry.hip calls these functions with its lane or thread index, scripts/sym_host_check.cpp runs the same text
// with the index as a loop variable under the host sanitizers.  Conventions of sm_lattice.h, whose reduction, enumeration, angle and
// determinant tests, wrap and 27-image pair cost are used as they stand: float64 or exact integers, every operation rounded separately,
// sqrt and floor the only library functions, so that tests/sym_ref64.py reproduces the bits.
//
// An operation is (W, t): f' = wrap(f W^-1 + t), W a lattice map of the reduced cell onto itself (rows of W L are the images of the
// axes).  W and W^-1 have the same determinant and, W being of finite order and similar to an orthogonal matrix, the same trace, so the
// class of the rotation part is read off W.
#pragma once
#include "sm_assign.h"

namespace mi {

enum { SYM_MAX_OPS = 192, SYM_MAX_TRANS = 64, SYM_INFO = 8, SYM_CLASSES = 10 };
enum {
    SYM_OK = 0,
    SYM_NOT_PREPARED = 1,
    SYM_BOX_CAP = 2,
    SYM_MAP_CAP = 4,
    SYM_NO_LATTICE = 8,
    SYM_AMBIGUOUS = 16,
    SYM_OPS_CAP = 32,
    SYM_NOT_A_GROUP = 64,
    SYM_PRIM_FAIL = 128,
    SYM_BAD_TOL = 256
};

#pragma clang fp contract(off)

SM_HD bool sym_tol_ok(double tol) { return tol >= 0.0 && tol <= 1.0; }

// the length rule of a self-map: absolute, in the prepared set's units
SM_HD bool sym_length_ok(double len, double target, double tol) { return sm_abs(len - target) <= tol; }

// the matcher's box with the relative tolerance tol / (the shortest axis): (1 + tol / min) max >= max + tol, so it holds every vector
// the length rule admits
SM_HD int sym_box(const SmTarget& t, const double* inv, double tol, int* bound) {
    double mn = t.len[0] < t.len[1] ? t.len[0] : t.len[1];
    mn = mn < t.len[2] ? mn : t.len[2];
    return sm_box(t, inv, tol / mn, bound);
}

// the rigid metric G = L L^T (all nine written)
SM_HD void sym_metric(const double* L, double* G) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) G[3 * i + j] = sm_dot3(L + 3 * i, L + 3 * j);
}

SM_HD bool sym_is_identity(const int* M) {
    return M[0] == 1 && M[1] == 0 && M[2] == 0 && M[3] == 0 && M[4] == 1 && M[5] == 0 && M[6] == 0 && M[7] == 0 && M[8] == 1;
}

// The atom of the block [b0, b0 + nb) of f nearest to the image img + t: the first minimum in ascending order of the 27-image pair cost.
// u: image - atom (+ the lattice vector of the minimum); d2: the squared distance, clamped at 0.
SM_HD int sym_nearest(const double* G, const double* f, int b0, int nb, const double* img, const double* t, double* u, double* d2) {
    double best = sm_inf();
    int at = b0;
    u[0] = u[1] = u[2] = 0.0;
    for (int b = b0; b < b0 + nb; ++b) {
        double uu[3];
        const double c = sm_pair_cost(G, f + 3 * b, img, t, uu);
        if (c < best) best = c, at = b, u[0] = uu[0], u[1] = uu[1], u[2] = uu[2];
    }
    *d2 = best > 0.0 ? best : 0.0;
    return at;
}

// the class of a rotation part by (determinant, trace): the index of -6, -4, -3, -2, -1, 1, 2, 3, 4, 6 in that order, or -1
SM_HD int sym_class(const int* M) {
    const int d = sm_idet3(M), tr = M[0] + M[4] + M[8];
    if (d == 1) return tr == 3 ? 5 : (tr == -1 ? 6 : (tr == 0 ? 7 : (tr == 1 ? 8 : (tr == 2 ? 9 : -1))));
    if (d == -1) return tr == -3 ? 4 : (tr == 1 ? 3 : (tr == 0 ? 2 : (tr == -1 ? 1 : (tr == -2 ? 0 : -1))));
    return -1;
}

// a histogram as one integer, four bits a class (no class of a point group has more than 9 members)
SM_HD constexpr uint64_t sym_row(int n6, int n4, int n3, int n2, int n1, int p1, int p2, int p3, int p4, int p6) {
    return (uint64_t)n6 | (uint64_t)n4 << 4 | (uint64_t)n3 << 8 | (uint64_t)n2 << 12 | (uint64_t)n1 << 16 | (uint64_t)p1 << 20 | (uint64_t)p2 << 24 |
           (uint64_t)p3 << 28 | (uint64_t)p4 << 32 | (uint64_t)p6 << 36;
}
#define SYM_ROW(n6, n4, n3, n2, n1, p1, p2, p3, p4, p6) sym_row(n6, n4, n3, n2, n1, p1, p2, p3, p4, p6)

// The point group of a histogram: 1 .. 32, or 0.  The rows are the class counts -6, -4, -3, -2, -1, 1, 2, 3, 4, 6 of the 32 crystallographic
// point groups; tests/test_symmetry_host.py derives them by closing generator sets and compares them with this text.
SM_HD int sym_point_group(const int* hist) {
    uint64_t key = 0;
    bool big = false;
#pragma unroll
    for (int c = 0; c < SYM_CLASSES; ++c) big = big || hist[c] > 15 || hist[c] < 0, key |= (uint64_t)(hist[c] & 15) << (4 * c);
    if (big) return 0;
    int pg = 0;
#define SYM_PG(index, row) pg = key == (row) ? (index) : pg
    SYM_PG(1, SYM_ROW(0, 0, 0, 0, 0, 1, 0, 0, 0, 0));    // 1
    SYM_PG(2, SYM_ROW(0, 0, 0, 0, 1, 1, 0, 0, 0, 0));    // -1
    SYM_PG(3, SYM_ROW(0, 0, 0, 0, 0, 1, 1, 0, 0, 0));    // 2
    SYM_PG(4, SYM_ROW(0, 0, 0, 1, 0, 1, 0, 0, 0, 0));    // m
    SYM_PG(5, SYM_ROW(0, 0, 0, 1, 1, 1, 1, 0, 0, 0));    // 2/m
    SYM_PG(6, SYM_ROW(0, 0, 0, 0, 0, 1, 3, 0, 0, 0));    // 222
    SYM_PG(7, SYM_ROW(0, 0, 0, 2, 0, 1, 1, 0, 0, 0));    // mm2
    SYM_PG(8, SYM_ROW(0, 0, 0, 3, 1, 1, 3, 0, 0, 0));    // mmm
    SYM_PG(9, SYM_ROW(0, 0, 0, 0, 0, 1, 1, 0, 2, 0));    // 4
    SYM_PG(10, SYM_ROW(0, 2, 0, 0, 0, 1, 1, 0, 0, 0));   // -4
    SYM_PG(11, SYM_ROW(0, 2, 0, 1, 1, 1, 1, 0, 2, 0));   // 4/m
    SYM_PG(12, SYM_ROW(0, 0, 0, 0, 0, 1, 5, 0, 2, 0));   // 422
    SYM_PG(13, SYM_ROW(0, 0, 0, 4, 0, 1, 1, 0, 2, 0));   // 4mm
    SYM_PG(14, SYM_ROW(0, 2, 0, 2, 0, 1, 3, 0, 0, 0));   // -42m
    SYM_PG(15, SYM_ROW(0, 2, 0, 5, 1, 1, 5, 0, 2, 0));   // 4/mmm
    SYM_PG(16, SYM_ROW(0, 0, 0, 0, 0, 1, 0, 2, 0, 0));   // 3
    SYM_PG(17, SYM_ROW(0, 0, 2, 0, 1, 1, 0, 2, 0, 0));   // -3
    SYM_PG(18, SYM_ROW(0, 0, 0, 0, 0, 1, 3, 2, 0, 0));   // 32
    SYM_PG(19, SYM_ROW(0, 0, 0, 3, 0, 1, 0, 2, 0, 0));   // 3m
    SYM_PG(20, SYM_ROW(0, 0, 2, 3, 1, 1, 3, 2, 0, 0));   // -3m
    SYM_PG(21, SYM_ROW(0, 0, 0, 0, 0, 1, 1, 2, 0, 2));   // 6
    SYM_PG(22, SYM_ROW(2, 0, 0, 1, 0, 1, 0, 2, 0, 0));   // -6
    SYM_PG(23, SYM_ROW(2, 0, 2, 1, 1, 1, 1, 2, 0, 2));   // 6/m
    SYM_PG(24, SYM_ROW(0, 0, 0, 0, 0, 1, 7, 2, 0, 2));   // 622
    SYM_PG(25, SYM_ROW(0, 0, 0, 6, 0, 1, 1, 2, 0, 2));   // 6mm
    SYM_PG(26, SYM_ROW(2, 0, 0, 4, 0, 1, 3, 2, 0, 0));   // -6m2
    SYM_PG(27, SYM_ROW(2, 0, 2, 7, 1, 1, 7, 2, 0, 2));   // 6/mmm
    SYM_PG(28, SYM_ROW(0, 0, 0, 0, 0, 1, 3, 8, 0, 0));   // 23
    SYM_PG(29, SYM_ROW(0, 0, 8, 3, 1, 1, 3, 8, 0, 0));   // m-3
    SYM_PG(30, SYM_ROW(0, 0, 0, 0, 0, 1, 9, 8, 6, 0));   // 432
    SYM_PG(31, SYM_ROW(0, 6, 0, 6, 0, 1, 3, 8, 0, 0));   // -43m
    SYM_PG(32, SYM_ROW(0, 6, 8, 9, 1, 1, 9, 8, 6, 0));   // m-3m
#undef SYM_PG
    return pg;
}

// 1 triclinic, 2 monoclinic, 3 orthorhombic, 4 tetragonal, 5 trigonal, 6 hexagonal, 7 cubic; 0 for no point group
SM_HD int sym_crystal_system(int pg) {
    return pg < 1 ? 0 : (pg <= 2 ? 1 : (pg <= 5 ? 2 : (pg <= 8 ? 3 : (pg <= 15 ? 4 : (pg <= 20 ? 5 : (pg <= 27 ? 6 : 7))))));
}

// ---- the primitive cell ------------------------------------------------------------------------------------------------------------------
// a component of a translation in [-1/2, 1/2)
SM_HD double sym_centre(double x) { return x - floor(x + 0.5); }

// candidate e of the basis search: the centred refined translations, then the three unit vectors
SM_HD void sym_prim_cand(const double* ptrans, int ntr, int e, double* v) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = e < ntr ? sym_centre(ptrans[3 * e + c]) : (e - ntr == c ? 1.0 : 0.0);
}

// the triple generates the translation lattice: its index is n_trans
SM_HD bool sym_prim_det_ok(double det, int ntr) { return sm_abs(sm_abs(det) * (double)ntr - 1.0) < 0.1; }

SM_HD double sym_prim_det(const double* ptrans, int ntr, int i, int j, int k, double* P) {
    sym_prim_cand(ptrans, ntr, i, P), sym_prim_cand(ptrans, ntr, j, P + 3), sym_prim_cand(ptrans, ntr, k, P + 6);
    return sm_det3(P);
}

// row i of P x Lr
SM_HD void sym_prim_row(const double* P, const double* Lr, int i, double* row) {
#pragma unroll
    for (int c = 0; c < 3; ++c) row[c] = (P[3 * i] * Lr[c] + P[3 * i + 1] * Lr[3 + c]) + P[3 * i + 2] * Lr[6 + c];
}

// the coordinates of one atom in the primitive basis as float32 in [0, 1): wrap(f P^-1), a float that rounds to 1 is 0
SM_HD void sym_prim_frac(const double* f, const double* Pinv, float* out) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float w = (float)sm_wrap01((f[0] * Pinv[c] + f[1] * Pinv[3 + c]) + f[2] * Pinv[6 + c]);
        out[c] = w >= 1.0f ? 0.0f : w;
    }
}

}  // namespace mi
