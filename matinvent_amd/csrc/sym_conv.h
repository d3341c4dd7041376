// The arithmetic of the conventional cell (include/matinvent_hip_sym_conv.h), host and device: from the reduced cell of a
// primitive crystal and the rotation parts mi_sym_find returned for it to an integer basis M (rows: the conventional vectors in the reduced
// primitive basis), the centring vectors, the centring letter and the Bravais lattice.  sym_conv.hip calls these functions with its lane
// index, scripts/sym_conv_host_check.cpp runs the same text with the index as a loop variable under the host sanitizers.  Conventions of
// sym_ops.h and sm_lattice.h: float64 or exact integers, every operation rounded separately, only + - x / in a written order, so that
// tests/conv_ref64.py reproduces the bits.
//
// An operation acts as f' = f W^-1 + t, so the lattice vector with integer row k maps to k W^-1; W^-1 is in the group with W, so k P is
// the image of k under an operation of the group for every proper part P = det(W) W.
#pragma once
#include "sym_ops.h"

namespace mi {

enum { SYM_CONV_FAIL = 512 };
enum { CONV_INFO = 8, CONV_BOX = 2, CONV_MAX_MULT = 4, CONV_Q_MAX = 1 << 14, CONV_NO_POINT = 0x7fffffff };
enum { CONV_NONE = 0, CONV_P = 1, CONV_A = 2, CONV_B = 3, CONV_C = 4, CONV_I = 5, CONV_F = 6, CONV_R = 7 };
enum { CONV_MAX_AX2 = 9, CONV_MAX_AX3 = 4, CONV_MAX_AX4 = 3 };
enum { CONV_M_MAX = 8, CONV_T_MAX = 512 };   // 3 x 8 x 512 < CONV_Q_MAX, and 2 x CONV_Q_MAX^2 fits 32 bits

#pragma clang fp contract(off)

// C = A B (C is neither A nor B)
SM_HD void conv_imul(const int* A, const int* B, int* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// r = k A (a row times a matrix; r is not k)
SM_HD void conv_row_mul(const int* k, const int* A, int* r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = k[0] * A[c] + k[1] * A[3 + c] + k[2] * A[6 + c];
}

// the proper part P = det(W) W: -4 -> 4, -3 -> 3, -6 -> 6, m -> 2, -1 -> 1
SM_HD void conv_proper(const int* W, int* P) {
    const int d = sm_idet3(W);
#pragma unroll
    for (int i = 0; i < 9; ++i) P[i] = d * W[i];
}

// the order of P by repeated multiplication: 1, 2, 3, 4 or 6; 0 for anything else
SM_HD int conv_order(const int* P) {
    int M[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) M[i] = P[i];
    for (int n = 1; n <= 6; ++n) {
        if (sym_is_identity(M)) return n == 5 ? 0 : n;
        int Q[9];
        conv_imul(M, P, Q);
        bool big = false;
#pragma unroll
        for (int i = 0; i < 9; ++i) big = big || Q[i] > CONV_Q_MAX || Q[i] < -CONV_Q_MAX, M[i] = Q[i];
        if (big) return 0;
    }
    return 0;
}

// S = I + P + .. + P^(n-1): every row is a multiple of the axis, and an integer row k is perpendicular to the axis iff k S = 0
SM_HD void conv_axis_sum(const int* P, int n, int* S) {
    int M[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) S[i] = 0, M[i] = (i % 4 == 0) ? 1 : 0;
    for (int e = 0; e < n; ++e) {
        int Q[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) S[i] += M[i];
        conv_imul(M, P, Q);
#pragma unroll
        for (int i = 0; i < 9; ++i) M[i] = Q[i];
    }
}

SM_HD int conv_gcd(int a, int b) {
    a = a < 0 ? -a : a, b = b < 0 ? -b : b;
    while (b != 0) {
        const int r = a % b;
        a = b, b = r;
    }
    return a;
}

// the axis: the first non-zero row of S over its gcd, the first non-zero entry positive; false when S = 0
SM_HD bool conv_axis(const int* S, int* k) {
    const bool z0 = S[0] == 0 && S[1] == 0 && S[2] == 0, z1 = S[3] == 0 && S[4] == 0 && S[5] == 0;
    const int m0 = z0 ? 0 : 1, m1 = z0 && !z1 ? 1 : 0, m2 = z0 && z1 ? 1 : 0;
    int r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = (S[c] * m0 + S[3 + c] * m1) + S[6 + c] * m2;   // (the row by weights 0 / 1: no index into S)
    k[0] = k[1] = k[2] = 0;
    if (r[0] == 0 && r[1] == 0 && r[2] == 0) return false;
    const int g = conv_gcd(conv_gcd(r[0], r[1]), r[2]);
    const int lead = r[0] != 0 ? r[0] : (r[1] != 0 ? r[1] : r[2]);
    const int s = lead < 0 ? -g : g;
#pragma unroll
    for (int c = 0; c < 3; ++c) k[c] = r[c] / s;
    return true;
}

// one rotation part: the order of its proper part (0: none of 1, 2, 3, 4, 6, or no axis) and, for an order above 1, the axis
SM_HD void conv_classify(const int* W, int* order, int* axis) {
    int P[9], S[9];
    conv_proper(W, P);
    int n = conv_order(P);
    axis[0] = axis[1] = axis[2] = 0;
    if (n >= 2) {
        conv_axis_sum(P, n, S);
        if (!conv_axis(S, axis)) n = 0;
    }
    *order = n;
}

// the distinct axes by order, in operation order, and the first operation of the orders 3, 4 and 6
struct ConvAxes {
    int n2, n3, n4;
    int ax2[CONV_MAX_AX2 * 3], ax3[CONV_MAX_AX3 * 3], ax4[CONV_MAX_AX4 * 3];
    int first2, first3, first4, first6;
    bool bad;   // a part of no order, or more axes of an order than any point group has
};

SM_HD bool conv_axis_add(int* list, int* count, int cap, const int* k) {
    for (int e = 0; e < *count; ++e)
        if (list[3 * e] == k[0] && list[3 * e + 1] == k[1] && list[3 * e + 2] == k[2]) return true;
    if (*count >= cap) return false;
    list[3 * *count] = k[0], list[3 * *count + 1] = k[1], list[3 * *count + 2] = k[2];
    ++*count;
    return true;
}

SM_HD void conv_collect_begin(ConvAxes* ax) {
    ax->n2 = ax->n3 = ax->n4 = 0, ax->first2 = ax->first3 = ax->first4 = ax->first6 = -1, ax->bad = false;
    for (int i = 0; i < CONV_MAX_AX2 * 3; ++i) ax->ax2[i] = 0;
    for (int i = 0; i < CONV_MAX_AX3 * 3; ++i) ax->ax3[i] = 0;
    for (int i = 0; i < CONV_MAX_AX4 * 3; ++i) ax->ax4[i] = 0;
}

// operation i with a rotation part the operation before it did not have: order (of conv_classify; -1: no such part) and axis
SM_HD void conv_collect(ConvAxes* ax, int i, int order, const int* axis) {
    if (order < 0 || order == 1) return;
    if (order == 0) ax->bad = true;
    if (order == 2) {
        if (ax->first2 < 0) ax->first2 = i;
        if (!conv_axis_add(ax->ax2, &ax->n2, CONV_MAX_AX2, axis)) ax->bad = true;
    }
    if (order == 3) {
        if (ax->first3 < 0) ax->first3 = i;
        if (!conv_axis_add(ax->ax3, &ax->n3, CONV_MAX_AX3, axis)) ax->bad = true;
    }
    if (order == 4) {
        if (ax->first4 < 0) ax->first4 = i;
        if (!conv_axis_add(ax->ax4, &ax->n4, CONV_MAX_AX4, axis)) ax->bad = true;
    }
    if (order == 6 && ax->first6 < 0) ax->first6 = i;
}

// a G b^T: the rows a G first, each product and sum rounded on its own
SM_HD double conv_gdot(const double* G, const int* a, const int* b) {
    const double a0 = (double)a[0], a1 = (double)a[1], a2 = (double)a[2];
    const double v0 = (a0 * G[0] + a1 * G[3]) + a2 * G[6], v1 = (a0 * G[1] + a1 * G[4]) + a2 * G[7], v2 = (a0 * G[2] + a1 * G[5]) + a2 * G[8];
    return (v0 * (double)b[0] + v1 * (double)b[1]) + v2 * (double)b[2];
}

// point p of the box [-box, box]^3: the lower index is the lexicographically larger k, so of two vectors of equal length (k and -k among
// them) the minimum of (length, index) keeps the larger
SM_HD void conv_box_k(int p, int box, int* k) {
    const int side = 2 * box + 1;
    k[0] = box - p / (side * side), k[1] = box - (p / side) % side, k[2] = box - p % side;
}

SM_HD bool conv_parallel(const int* a, const int* b) {
    return a[1] * b[2] - a[2] * b[1] == 0 && a[2] * b[0] - a[0] * b[2] == 0 && a[0] * b[1] - a[1] * b[0] == 0;
}

// candidate p of a search: non-zero, perpendicular to the axis of S (k S = 0, exact) and, with use_excl, not parallel to excl; l2 = k G k^T
SM_HD bool conv_cand(int p, int box, const int* S, const int* excl, bool use_excl, const double* G, double* l2) {
    int k[3], r[3];
    conv_box_k(p, box, k);
    *l2 = 0.0;
    if (k[0] == 0 && k[1] == 0 && k[2] == 0) return false;
    conv_row_mul(k, S, r);
    if (r[0] != 0 || r[1] != 0 || r[2] != 0) return false;
    if (use_excl && conv_parallel(k, excl)) return false;
    *l2 = conv_gdot(G, k, k);
    return true;
}

SM_HD bool conv_lex_less(const int* x, const int* y) { return x[0] != y[0] ? x[0] < y[0] : (x[1] != y[1] ? x[1] < y[1] : x[2] < y[2]); }

// exchange two rows and their keys
SM_HD void conv_swap_if(bool swap, int* x, int* y, double* kx, double* ky) {
    if (!swap) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int t = x[c];
        x[c] = y[c], y[c] = t;
    }
    const double k = *kx;
    *kx = *ky, *ky = k;
}

SM_HD void conv_set_row(int* M, int i, const int* k) { M[3 * i] = k[0], M[3 * i + 1] = k[1], M[3 * i + 2] = k[2]; }

// The basis by crystal system.  rot: the crystal's operations' rotation parts [.][9].  search(S, excl, use_excl): the point of the box with the
// smallest (l2, index) among the candidates of conv_cand, or -1 -- a serial loop on the host, one fixed tree over the lanes on the device,
// the same pair either way.  Returns false on a failure; M is then not meaningful.
template <class Search>
SM_HD bool conv_basis(int system, const ConvAxes& ax, const int* rot, const double* G, int box, const Search& search, int* M, int* n_axes) {
    int P[9], S[9], a[3], b[3], c[3];
    *n_axes = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) M[i] = (i % 4 == 0) ? 1 : 0;
    if (ax.bad) return false;
    if (system == 1) return true;
    if (system == 2) {   // b the one two-fold axis; a, c the two shortest vectors of the plane perpendicular to it; beta >= 90 degrees
        *n_axes = ax.n2;
        if (ax.n2 != 1 || ax.first2 < 0) return false;
        conv_proper(rot + 9 * ax.first2, P);
        conv_axis_sum(P, 2, S);
        const int pa = search(S, S, false);
        if (pa < 0) return false;
        conv_box_k(pa, box, a);
        const int pc = search(S, a, true);
        if (pc < 0) return false;
        conv_box_k(pc, box, c);
        if (conv_gdot(G, a, c) > 0.0) c[0] = -c[0], c[1] = -c[1], c[2] = -c[2];
        conv_set_row(M, 0, a), conv_set_row(M, 1, ax.ax2), conv_set_row(M, 2, c);
        return true;
    }
    if (system == 3) {   // the three two-fold axes, a <= b <= c (of equal lengths the earlier axis first)
        *n_axes = ax.n2;
        if (ax.n2 != 3) return false;
        int r[9];
        double l2[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) r[e] = ax.ax2[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) l2[e] = conv_gdot(G, r + 3 * e, r + 3 * e);
        conv_swap_if(l2[1] < l2[0], r, r + 3, l2, l2 + 1);
        conv_swap_if(l2[2] < l2[1], r + 3, r + 6, l2 + 1, l2 + 2);
        conv_swap_if(l2[1] < l2[0], r, r + 3, l2, l2 + 1);
#pragma unroll
        for (int e = 0; e < 9; ++e) M[e] = r[e];
        return true;
    }
    if (system == 4 || system == 5 || system == 6) {   // c the main axis, a the shortest vector perpendicular to it, b its image
        int order = 4;
        if (system == 4) {
            *n_axes = ax.n4;
            if (ax.n4 != 1 || ax.first4 < 0) return false;
            conv_proper(rot + 9 * ax.first4, P);
        } else {
            order = 3;
            *n_axes = ax.n3;
            if (ax.n3 > 1) return false;
            if (ax.first3 >= 0) {
                conv_proper(rot + 9 * ax.first3, P);
            } else {   // only an order 6: its square
                if (ax.first6 < 0) return false;
                int P6[9];
                conv_proper(rot + 9 * ax.first6, P6);
                conv_imul(P6, P6, P);
                *n_axes = 1;
            }
        }
        conv_axis_sum(P, order, S);
        if (!conv_axis(S, c)) return false;
        const int pa = search(S, S, false);
        if (pa < 0) return false;
        conv_box_k(pa, box, a);
        conv_row_mul(a, P, b);
        conv_set_row(M, 0, a), conv_set_row(M, 1, b), conv_set_row(M, 2, c);
        return true;
    }
    if (system == 7) {   // the three four-fold axes, without them (23, m-3) the three two-fold ones, in descending lexicographic order
        const bool four = ax.n4 > 0;
        const int* list = four ? ax.ax4 : ax.ax2;
        *n_axes = four ? ax.n4 : ax.n2;
        if (*n_axes != 3) return false;
        int r[9];
        double unused[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int e = 0; e < 9; ++e) r[e] = list[e];
        conv_swap_if(conv_lex_less(r, r + 3), r, r + 3, unused, unused + 1);
        conv_swap_if(conv_lex_less(r + 3, r + 6), r + 3, r + 6, unused + 1, unused + 2);
        conv_swap_if(conv_lex_less(r, r + 3), r, r + 3, unused, unused + 1);
#pragma unroll
        for (int e = 0; e < 9; ++e) M[e] = r[e];
        return true;
    }
    return false;
}

// det M > 0 by the sign of c -- of b in the monoclinic system, where the sign of c is taken by beta >= 90 degrees and that of the axis is
// free; returns the determinant (0: no basis)
SM_HD int conv_orient(int system, int* M) {
    int d = sm_idet3(M);
    if (d < 0) {
        if (system == 2) M[3] = -M[3], M[4] = -M[4], M[5] = -M[5];
        else M[6] = -M[6], M[7] = -M[7], M[8] = -M[8];
        d = -d;
    }
    return d;
}

// The centring vectors as numerators over d = det M (1 .. 4): the distinct k adj(M) mod d over k in {0 .. d-1}^3, in ascending
// lexicographic order (zero first).  Returns their number, which is d for a basis of a sublattice of index d; -1 past CONV_MAX_MULT.
SM_HD int conv_centring_vectors(const int* M, int d, int* cvec) {
    int A[9], count = 0;
    sm_iadj3(M, A);
#pragma unroll
    for (int i = 0; i < CONV_MAX_MULT * 3; ++i) cvec[i] = 0;
    for (int k0 = 0; k0 < d; ++k0)
        for (int k1 = 0; k1 < d; ++k1)
            for (int k2 = 0; k2 < d; ++k2) {
                const int k[3] = {k0, k1, k2};
                int v[3];
                conv_row_mul(k, A, v);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = ((v[c] % d) + d) % d;
                int at = 0;   // the place of v in the ascending list
                bool have = false;
                for (int e = 0; e < count; ++e) {
                    const int* w = cvec + 3 * e;
                    const bool same = w[0] == v[0] && w[1] == v[1] && w[2] == v[2];
                    const bool below = conv_lex_less(w, v);
                    have = have || same;
                    at += below ? 1 : 0;
                }
                if (have) continue;
                if (count >= CONV_MAX_MULT) return -1;
                for (int e = count; e > at; --e) cvec[3 * e] = cvec[3 * e - 3], cvec[3 * e + 1] = cvec[3 * e - 2], cvec[3 * e + 2] = cvec[3 * e - 1];
                cvec[3 * at] = v[0], cvec[3 * at + 1] = v[1], cvec[3 * at + 2] = v[2];
                ++count;
            }
    return count;
}

SM_HD bool conv_vec_is(const int* v, int x, int y, int z) { return v[0] == x && v[1] == y && v[2] == z; }

// the letter of a vector set (count vectors over d); reverse: the set is the reverse rhombohedral one
SM_HD int conv_centring_name(int d, int count, const int* cvec, bool* reverse) {
    *reverse = false;
    if (count != d || !conv_vec_is(cvec, 0, 0, 0)) return CONV_NONE;
    if (d == 1) return CONV_P;
    if (d == 2) return conv_vec_is(cvec + 3, 1, 1, 1) ? CONV_I : (conv_vec_is(cvec + 3, 1, 1, 0) ? CONV_C : (conv_vec_is(cvec + 3, 1, 0, 1) ? CONV_B : (conv_vec_is(cvec + 3, 0, 1, 1) ? CONV_A : CONV_NONE)));
    if (d == 3) {
        if (conv_vec_is(cvec + 3, 1, 2, 2) && conv_vec_is(cvec + 6, 2, 1, 1)) return CONV_R;
        if (conv_vec_is(cvec + 3, 1, 2, 1) && conv_vec_is(cvec + 6, 2, 1, 2)) {
            *reverse = true;
            return CONV_R;
        }
        return CONV_NONE;
    }
    if (d == 4) return conv_vec_is(cvec + 3, 0, 2, 2) && conv_vec_is(cvec + 6, 2, 0, 2) && conv_vec_is(cvec + 9, 2, 2, 0) ? CONV_F : CONV_NONE;
    return CONV_NONE;
}

// 1 .. 14 in the order aP mP mS oP oS oI oF tP tI hR hP cP cI cF; 0: the centring is not one of the system
SM_HD int conv_bravais(int system, int centring) {
    if (system == 1) return centring == CONV_P ? 1 : 0;
    if (system == 2) return centring == CONV_P ? 2 : (centring == CONV_A || centring == CONV_C || centring == CONV_I ? 3 : 0);
    if (system == 3) return centring == CONV_P ? 4 : (centring == CONV_C ? 5 : (centring == CONV_I ? 6 : (centring == CONV_F ? 7 : 0)));
    if (system == 4) return centring == CONV_P ? 8 : (centring == CONV_I ? 9 : 0);
    if (system == 5) return centring == CONV_R ? 10 : (centring == CONV_P ? 11 : 0);
    if (system == 6) return centring == CONV_P ? 11 : 0;
    if (system == 7) return centring == CONV_P ? 12 : (centring == CONV_I ? 13 : (centring == CONV_F ? 14 : 0));
    return 0;
}

// From the basis of conv_basis to the oriented basis, its centring and the Bravais index; 0 on a failure.  An orthorhombic cell centred on
// the bc or the ac face is permuted so that the centred face is ab (a <= b stays); a reverse rhombohedral setting is turned obverse by
// negating a and b.
SM_HD int conv_finish(int system, int* M, int* mult, int* centring, int* cvec) {
    *mult = 1, *centring = CONV_NONE;
    for (int round = 0; round < 2; ++round) {
        const int d = conv_orient(system, M);
        if (d < 1 || d > CONV_MAX_MULT) return 0;
        bool reverse;
        const int count = conv_centring_vectors(M, d, cvec);
        const int name = conv_centring_name(d, count, cvec, &reverse);
        if (name == CONV_NONE) return 0;
        if (round == 0 && system == 3 && (name == CONV_A || name == CONV_B)) {
            int R[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = M[i];
            if (name == CONV_A) conv_set_row(M, 0, R + 3), conv_set_row(M, 1, R + 6), conv_set_row(M, 2, R);   // (b, c, a)
            else conv_set_row(M, 1, R + 6), conv_set_row(M, 2, R + 3);                                             // (a, c, b)
            continue;
        }
        if (round == 0 && name == CONV_R && reverse) {
#pragma unroll
            for (int i = 0; i < 6; ++i) M[i] = -M[i];
            continue;
        }
        if (reverse) return 0;
        *mult = d, *centring = name;
        return conv_bravais(system, name);
    }
    return 0;
}

SM_HD int conv_max_abs(const int* M) {
    int m = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) m = (M[i] < 0 ? -M[i] : M[i]) > m ? (M[i] < 0 ? -M[i] : M[i]) : m;
    return m;
}

// Q = M T and adj(Q) (Q^-1 = adj(Q) / mult, det T = 1); false when an entry of Q leaves the range in which adj(Q) is exact in 32 bits
SM_HD bool conv_transform(const int* M, const int* T, int* adj) {
    int Q[9];
    bool big = false;
#pragma unroll
    for (int i = 0; i < 9; ++i) big = big || T[i] > CONV_T_MAX || T[i] < -CONV_T_MAX || M[i] > CONV_M_MAX || M[i] < -CONV_M_MAX;
    if (big) return false;
    conv_imul(M, T, Q);
    sm_iadj3(Q, adj);
    return true;
}

// the coordinates of copy j of one atom in the conventional basis as float32 in [0, 1): wrap((f adj(Q) + v_j) / mult), a float that rounds
// to 1 is 0
SM_HD void conv_frac(const float* f32, const int* adj, const int* v, int mult, float* out) {
    const double f0 = (double)f32[0], f1 = (double)f32[1], f2 = (double)f32[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double x = (f0 * (double)adj[c] + f1 * (double)adj[3 + c]) + f2 * (double)adj[6 + c];
        const float w = (float)sm_wrap01((x + (double)v[c]) / (double)mult);
        out[c] = w >= 1.0f ? 0.0f : w;
    }
}

// row i of M x Lr as float64
SM_HD void conv_lat_row(const int* M, const double* Lr, int i, double* row) {
#pragma unroll
    for (int c = 0; c < 3; ++c) row[c] = ((double)M[3 * i] * Lr[c] + (double)M[3 * i + 1] * Lr[3 + c]) + (double)M[3 * i + 2] * Lr[6 + c];
}

}  // namespace mi
