// The arithmetic of the substrate matcher (include/matinvent_hip_zsl.h), host and device: plane bases, the pair reduction,
// superlattice entries, the admissibility and match rules and the packed tie key.  zsl.hip calls these functions with its thread index,
// scripts/zsl_host_check.cpp runs the same text with the index as a loop variable under the host sanitizers.  Everything is float64 (or
// exact integers) and every product and addition is rounded separately (no contraction into FMAs).  The library functions are sqrt and
// floor (exact) and acos, whose last bits may differ between host and device: theta and the angle strain are compared to a tolerance,
// every integer and every area bit for bit (tests/zsl_ref64.py reports the margin of every decision theta enters).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZSL_HD __host__ __device__ inline
#else
#define ZSL_HD inline
#endif

namespace mi {

enum { ZSL_MAX_MULT = 63, ZSL_MAX_MILLER = 8, ZSL_REDUCE_ITERS = 64, ZSL_THREADS = 256, ZSL_MAX_HNF = 168, ZSL_TABLE = 3276, ZSL_ROW_D = 10, ZSL_ROW_I = 20 };
enum { ZSL_OK = 0, ZSL_NO_MATCH = 1, ZSL_MULT_CAP = 2, ZSL_REDUCE_CAP = 3, ZSL_BAD_CELL = 4 };
enum { ZSL_NO_KEY = 0x7fffffff };

#pragma clang fp contract(off)

ZSL_HD bool zsl_finite(double v) { return v - v == 0.0; }
ZSL_HD double zsl_inf() { return (double)__builtin_inff(); }
ZSL_HD double zsl_nan() { return (double)__builtin_nanf(""); }
ZSL_HD double zsl_abs(double v) { return v < 0.0 ? -v : v; }
ZSL_HD int zsl_max(int a, int b) { return a > b ? a : b; }
ZSL_HD double zsl_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// sigma(n): the number of Hermite normal forms [[i, j], [0, n / i]] of determinant n
ZSL_HD constexpr int zsl_sigma(int n) {
    int s = 0;
    for (int d = 1; d <= n; ++d) s += n % d == 0 ? n / d : 0;
    return s;
}
// the first entry of multiple n in a plane's table
ZSL_HD constexpr int zsl_offset(int n) {
    int s = 0;
    for (int k = 1; k < n; ++k) s += zsl_sigma(k);
    return s;
}
static_assert(zsl_offset(ZSL_MAX_MULT + 1) == ZSL_TABLE && zsl_sigma(60) == ZSL_MAX_HNF, "table sizes");

// sigma(n) and the offsets for n = 1 .. ZSL_MAX_MULT + 1 as a compile-time table (entry 0 unused)
struct ZslCounts {
    int sig[ZSL_MAX_MULT + 2], off[ZSL_MAX_MULT + 2];
};
ZSL_HD constexpr ZslCounts zsl_counts() {
    ZslCounts c{};
    for (int n = 1; n <= ZSL_MAX_MULT + 1; ++n) c.sig[n] = zsl_sigma(n), c.off[n] = zsl_offset(n);
    return c;
}

// HNF number idx of determinant n: i ascending over the divisors, j = 0 .. n/i - 1
ZSL_HD void zsl_hnf(int n, int idx, int* i, int* j, int* m) {
    *i = 0, *j = 0, *m = 0;
    for (int d = 1; d <= n; ++d) {
        if (n % d != 0) continue;
        const int w = n / d;
        if (idx < w) {
            *i = d, *j = idx, *m = w;
            return;
        }
        idx -= w;
    }
}

// extended Euclid with truncating division: g = gcd(h, k) > 0 (h, k not both zero) and p h + q k = g
ZSL_HD int zsl_egcd(int h, int k, int* p, int* q) {
    int r0 = h, r1 = k, s0 = 1, s1 = 0, t0 = 0, t1 = 1;
    while (r1 != 0) {
        const int qu = r0 / r1;
        const int r2 = r0 - qu * r1, s2 = s0 - qu * s1, t2 = t0 - qu * t1;
        r0 = r1, r1 = r2, s0 = s1, s1 = s2, t0 = t1, t1 = t2;
    }
    if (r0 < 0) r0 = -r0, s0 = -s0, t0 = -t0;
    *p = s0, *q = t0;
    return r0;
}

// the in-plane basis of (h, k, l): u x v = (h, k, l)
ZSL_HD void zsl_basis(const int* hkl, int* u, int* v) {
    const int h = hkl[0], k = hkl[1], l = hkl[2];
    if (h == 0 && k == 0) {
        u[0] = 1, u[1] = 0, u[2] = 0, v[0] = 0, v[1] = 1, v[2] = 0;
        return;
    }
    int p, q;
    const int g = zsl_egcd(h, k, &p, &q);
    u[0] = -k / g, u[1] = h / g, u[2] = 0;
    v[0] = -p * l, v[1] = -q * l, v[2] = g;
}

// x = u L (rows of L are the cell vectors)
ZSL_HD void zsl_cart(const int* u, const double* L, double* x) {
    for (int c = 0; c < 3; ++c) x[c] = ((double)u[0] * L[c] + (double)u[1] * L[3 + c]) + (double)u[2] * L[6 + c];
}

// The pair reduction: the first rule that applies, at most ZSL_REDUCE_ITERS applications; false past the cap.
ZSL_HD bool zsl_reduce(double* a, double* b) {
    for (int it = 0; it < ZSL_REDUCE_ITERS; ++it) {
        if (zsl_dot(a, b) < 0.0) {
            b[0] = -b[0], b[1] = -b[1], b[2] = -b[2];
            continue;
        }
        const double na = zsl_dot(a, a), nb = zsl_dot(b, b);
        if (na > nb) {
            for (int c = 0; c < 3; ++c) {
                const double t = a[c];
                a[c] = b[c], b[c] = t;
            }
            continue;
        }
        const double p[3] = {b[0] + a[0], b[1] + a[1], b[2] + a[2]};
        if (nb > zsl_dot(p, p)) {
            b[0] = p[0], b[1] = p[1], b[2] = p[2];
            continue;
        }
        const double m[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
        if (nb > zsl_dot(m, m)) {
            b[0] = m[0], b[1] = m[1], b[2] = m[2];
            continue;
        }
        return true;
    }
    return false;
}

ZSL_HD double zsl_area(const double* a, const double* b) {
    const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    return sqrt(zsl_dot(c, c));
}

// One plane of one cell: the reduced vectors vec[6], the area and the multiple count; returns the plane's status.
ZSL_HD int zsl_plane(const float* lat, const int* hkl, double max_area, double* vec, double* area, int* mult) {
    for (int i = 0; i < 6; ++i) vec[i] = 0.0;
    *area = 0.0, *mult = 0;
    double L[9];
    bool bad = false;
    for (int i = 0; i < 9; ++i) {
        L[i] = (double)lat[i];
        bad = bad || !zsl_finite(L[i]);
    }
    for (int i = 0; i < 3; ++i) bad = bad || hkl[i] > ZSL_MAX_MILLER || hkl[i] < -ZSL_MAX_MILLER;
    if (bad) return ZSL_BAD_CELL;
    const double det = (L[0] * (L[4] * L[8] - L[5] * L[7]) - L[1] * (L[3] * L[8] - L[5] * L[6])) + L[2] * (L[3] * L[7] - L[4] * L[6]);
    if (!(zsl_abs(det) > 0.0) || !zsl_finite(det)) return ZSL_BAD_CELL;
    int u[3], v[3];
    zsl_basis(hkl, u, v);
    double a[3], b[3];
    zsl_cart(u, L, a);
    zsl_cart(v, L, b);
    const bool ended = zsl_reduce(a, b);
    const double A = zsl_area(a, b);
    if (!(A > 0.0) || !zsl_finite(A)) return ZSL_BAD_CELL;
    const double q = max_area / A;
    const bool capped = !(q < (double)(ZSL_MAX_MULT + 1));
    for (int c = 0; c < 3; ++c) vec[c] = a[c], vec[3 + c] = b[c];
    *area = A;
    *mult = capped ? ZSL_MAX_MULT : (int)floor(q);
    return !ended ? ZSL_REDUCE_CAP : capped ? ZSL_MULT_CAP : ZSL_OK;
}

// The superlattice [[i, j], [0, m]] of the reduced pair (a, b) = vec: e = (|a'|, |b'|, theta'); false when its reduction passed the cap.
ZSL_HD bool zsl_super(const double* vec, int i, int j, int m, double* e) {
    double x[3], y[3];
    for (int c = 0; c < 3; ++c) {
        x[c] = (double)i * vec[c] + (double)j * vec[3 + c];
        y[c] = (double)m * vec[3 + c];
    }
    const bool ended = zsl_reduce(x, y);
    const double la = sqrt(zsl_dot(x, x)), lb = sqrt(zsl_dot(y, y));
    double cs = zsl_dot(x, y) / (la * lb);
    cs = cs > 1.0 ? 1.0 : cs < -1.0 ? -1.0 : cs;
    e[0] = la, e[1] = lb, e[2] = acos(cs);
    return ended;
}

ZSL_HD bool zsl_admissible(double Af, double As, int nf, int ns, double tol) { return zsl_abs(Af / As - (double)ns / (double)nf) < tol; }

// the match rule on two entries; s[3] the signed strains
ZSL_HD bool zsl_match(const double* f, const double* sub, double ltol, double atol, double* s) {
    s[0] = sub[0] / f[0] - 1.0, s[1] = sub[1] / f[1] - 1.0, s[2] = sub[2] / f[2] - 1.0;
    return zsl_abs(s[0]) <= ltol && zsl_abs(s[1]) <= ltol && zsl_abs(s[2]) <= atol;
}

ZSL_HD double zsl_strain(const double* s) {
    const double a = zsl_abs(s[0]), b = zsl_abs(s[1]), c = zsl_abs(s[2]);
    const double ab = a > b ? a : b;
    return ab > c ? ab : c;
}

// The tie key: (n_f, film HNF index, n_s, substrate HNF index) in 6 + 8 + 6 + 8 bits; integer order is the lexicographic order.
ZSL_HD int zsl_key(int nf, int h, int ns, int g) { return (nf << 22) | (h << 14) | (ns << 8) | g; }
ZSL_HD void zsl_unkey(int key, int* nf, int* h, int* ns, int* g) { *nf = key >> 22, *h = (key >> 14) & 255, *ns = (key >> 8) & 63, *g = key & 255; }

// the exact order of the least-strained argmin: the smaller strain, of equal strains the lower key
ZSL_HD bool zsl_better(double v, int k, double ov, int ok) { return v < ov || (v == ov && k < ok); }

// A match written into an item's rows: d[0 .. 3] = area, strains; r[0 .. 8] = film plane, n_f, n_s, the two HNFs.  key == ZSL_NO_KEY: none.
// off: ZslCounts::off.
ZSL_HD void zsl_write_match(int key, int fplane, const double* vec, double Af, const double* table, const int* off, double ltol, double atol, double* d, int* r) {
    if (key == ZSL_NO_KEY) {
        d[0] = zsl_inf(), d[1] = zsl_nan(), d[2] = zsl_nan(), d[3] = zsl_nan();
        r[0] = -1;
        for (int i = 1; i < 9; ++i) r[i] = 0;
        return;
    }
    int nf, h, ns, g;
    zsl_unkey(key, &nf, &h, &ns, &g);
    zsl_hnf(nf, h, &r[3], &r[4], &r[5]);
    zsl_hnf(ns, g, &r[6], &r[7], &r[8]);
    r[0] = fplane, r[1] = nf, r[2] = ns;
    double e[3], s[3];
    zsl_super(vec, r[3], r[4], r[5], e);
    zsl_match(e, table + 3 * (off[ns] + g), ltol, atol, s);
    d[0] = (double)nf * Af, d[1] = s[0], d[2] = s[1], d[3] = s[2];
}

}  // namespace mi
