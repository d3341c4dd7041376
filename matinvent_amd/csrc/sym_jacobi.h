// The arithmetic of mi_sym_eigvals (include/matinvent_hip_vib.h), host and device: the eigenvalues of a real symmetric matrix by
// cyclic Jacobi rotations in the round-robin (tournament) ordering.  vib.hip's kernel calls these functions, and scripts/vib_host_check.cpp
// runs the same text against plain loops under the host sanitizers.  Separately rounded float64 operations: no contraction into FMAs.
//
// One sweep of a matrix of order M is Me - 1 ROUNDS (Me: M rounded up to even) of Me / 2 disjoint pairs (p < q); a pair with q >= M is the
// bye of an odd M and is skipped.  A round:
//   1. every pair's rotation from the matrix BEFORE the round (jac_rotation): it rotates when a_pq != 0 and |a_pq| > eps sqrt|a_pp| sqrt|a_qq|,
//      with a_pq read from the upper triangle;
//   2. the column update  A <- A J:      a_ip' = c a_ip - s a_iq,  a_iq' = s a_ip + c a_iq   for every row i;
//   3. the row update     A <- J^T A:    a_pj' = c a_pj - s a_qj,  a_qj' = s a_pj + c a_qj   for every column j, except that the four
//      elements of a rotating pair's own 2 x 2 block are written from the values of step 1: a_pp - t a_pq, a_qq + t a_pq, 0, 0.
// Every element is written once per step from one formula of values of the step before, so the bits do not depend on how the elements are
// spread over threads.  A pair that does not rotate writes nothing, and a round in which no pair rotates is skipped.  The iteration stops
// after a sweep without a rotation; `sweeps` counts the sweeps that rotated.  The two triangles are rotated by formulas that differ in the
// order of their two steps, so they drift apart in the last place; the 2 x 2 block of a rotating pair is reset to exact symmetry.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JAC_HD __host__ __device__ inline
#else
#define JAC_HD inline
#endif

namespace mi {

enum { EIG_OK = 0, EIG_NO_CONVERGENCE = 1, EIG_BAD_INPUT = 2 };
enum { EIG_MAX_SWEEPS = 30, EIG_LDS_MAX_M = 128, EIG_MAX_M = 768 };
constexpr double EIG_EPS = 2.220446049250313e-16;   // 2^-52

#pragma clang fp contract(off)

JAC_HD bool jac_finite(double v) { return (__builtin_bit_cast(uint64_t, v) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }
JAC_HD double jac_nan() { return __builtin_bit_cast(double, (uint64_t)0x7FF8000000000000ull); }
JAC_HD int jac_even(int M) { return M + (M & 1); }

// pair k (0 .. Me / 2 - 1) of round r (0 .. Me - 2): player Me - 1 stays, the others move round a circle of Me - 1 seats
JAC_HD void jac_pair(int Me, int r, int k, int* p, int* q) {
    const int m = Me - 1;
    const int a = k == 0 ? m : (r + k) % m, b = k == 0 ? r : (r - k + m) % m;
    *p = a < b ? a : b;
    *q = a < b ? b : a;
}

struct JacRot {
    double c, s, pp, qq;   // pp, qq: the pair's new diagonal
    int rot;
};

JAC_HD JacRot jac_rotation(double app, double aqq, double apq) {
    JacRot R;
    R.c = 1.0, R.s = 0.0, R.pp = app, R.qq = aqq, R.rot = 0;
    if (apq != 0.0 && fabs(apq) > EIG_EPS * (sqrt(fabs(app)) * sqrt(fabs(aqq)))) {   // (two roots: the product a_pp a_qq may overflow)
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        R.c = 1.0 / sqrt(t * t + 1.0);
        R.s = t * R.c;
        R.pp = app - t * apq;
        R.qq = aqq + t * apq;
        R.rot = 1;
    }
    return R;
}

JAC_HD double jac_first(double c, double s, double x, double y) { return c * x - s * y; }    // the p side of a pair
JAC_HD double jac_second(double c, double s, double x, double y) { return s * x + c * y; }   // the q side

// the position of d[i] in the ascending order, ties to the lower index
JAC_HD int jac_rank(const double* A, int ld, int M, int i) {
    const double v = A[(size_t)i * ld + i];
    int r = 0;
    for (int j = 0; j < M; ++j) {
        const double w = A[(size_t)j * ld + j];
        r += (w < v || (w == v && j < i)) ? 1 : 0;
    }
    return r;
}

// One matrix, serially (the host check's form): A [M][M] is destroyed, evals [M] ascending.  Returns the status.
inline int jac_eigvals_host(int M, double* A, double* evals, int* sweeps, double* rc, double* rs, double* rpp, double* rqq, int* rrot) {
    for (size_t i = 0; i < (size_t)M * M; ++i)
        if (!jac_finite(A[i])) {
            for (int k = 0; k < M; ++k) evals[k] = jac_nan();
            *sweeps = 0;
            return EIG_BAD_INPUT;
        }
    const int Me = jac_even(M), np = Me / 2;
    int done = 0, status = EIG_NO_CONVERGENCE;
    for (int sw = 0; sw < EIG_MAX_SWEEPS; ++sw) {
        int any_sweep = 0;
        for (int r = 0; r < Me - 1; ++r) {
            int any = 0, p, q;
            for (int k = 0; k < np; ++k) {
                jac_pair(Me, r, k, &p, &q);
                rrot[k] = 0;
                if (q >= M) continue;
                const JacRot R = jac_rotation(A[(size_t)p * M + p], A[(size_t)q * M + q], A[(size_t)p * M + q]);
                rc[k] = R.c, rs[k] = R.s, rpp[k] = R.pp, rqq[k] = R.qq, rrot[k] = R.rot;
                any |= R.rot;
            }
            if (!any) continue;
            any_sweep = 1;
            for (int k = 0; k < np; ++k) {
                jac_pair(Me, r, k, &p, &q);
                if (q >= M || !rrot[k]) continue;
                for (int i = 0; i < M; ++i) {
                    const double x = A[(size_t)i * M + p], y = A[(size_t)i * M + q];
                    A[(size_t)i * M + p] = jac_first(rc[k], rs[k], x, y);
                    A[(size_t)i * M + q] = jac_second(rc[k], rs[k], x, y);
                }
            }
            for (int k = 0; k < np; ++k) {
                jac_pair(Me, r, k, &p, &q);
                if (q >= M || !rrot[k]) continue;
                for (int j = 0; j < M; ++j) {
                    const double x = A[(size_t)p * M + j], y = A[(size_t)q * M + j];
                    A[(size_t)p * M + j] = j == p ? rpp[k] : (j == q ? 0.0 : jac_first(rc[k], rs[k], x, y));
                    A[(size_t)q * M + j] = j == q ? rqq[k] : (j == p ? 0.0 : jac_second(rc[k], rs[k], x, y));
                }
            }
        }
        if (!any_sweep) {
            status = EIG_OK;
            break;
        }
        ++done;
    }
    *sweeps = done;
    for (int i = 0; i < M; ++i) evals[jac_rank(A, M, M, i)] = A[(size_t)i * M + i];
    return status;
}

}  // namespace mi
