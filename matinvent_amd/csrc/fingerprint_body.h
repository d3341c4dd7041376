// The structure-fingerprint kernel's body (include/matinvent_hip_fp.h), written as the phases between its barriers so that
// the very same source also compiles for the host, where a stand-alone program runs every phase as a loop over the thread index
// (scripts/fingerprint_host_check.cpp: bounds and guards under the host sanitizers).  Plain C++, no intrinsics beyond the two integer
// LDS additions behind fp_add().
#ifndef MI_FINGERPRINT_BODY_H
#define MI_FINGERPRINT_BODY_H

#include <cmath>
#include <cstdint>

#include "../../include/matinvent_hip_fp.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI_FP_FN __device__ __forceinline__
#else
#define MI_FP_FN static inline
#endif

namespace mi {

constexpr int FP_THREADS = 256;
constexpr int FP_ROW_MAX = MI_FP_MAX_BLOCKS * MI_FP_MAX_BINS;
constexpr float FP_SCALE = 4294967296.0f;              // 2^32: one count of the fixed-point histogram
constexpr double FP_INV_SCALE = 1.0 / 4294967296.0;

struct FpArgs {
    const int* node_off;     // [B + 1]
    const int* atom_types;   // [N]
    const float* frac;       // [N][3]
    const float* lattices;   // [B][9]
    float* out_fp;           // [B][MI_FP_MAX_BLOCKS * nbins]
    float* out_info;         // [B][4]
    float r_max, sigma;
    int nbins;
};

// one crystal's working set: LDS on the device (about 30 KB), an ordinary object on the host
struct FpShared {
    unsigned long long hist[FP_ROW_MAX];   // C_ab(k) in units of 2^-32
    float g[FP_ROW_MAX];                   // sqrt(w_ab) F_ab(k)
    float red[FP_THREADS];
    int cnt[101], slot[101];               // by atomic number: atoms of it, its rank among the crystal's species (-1: absent / beyond the 8th)
    int na[MI_FP_MAX_SPECIES];             // N_a by rank
    int blk_a[MI_FP_MAX_BLOCKS], blk_b[MI_FP_MAX_BLOCKS];
    float L[9];
    int reach[3];
    int bad_type, bad_coord, status, m;
    float V, norm, images;
};

MI_FP_FN void fp_add(int* p, int v) {
#if defined(__HIPCC__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}

MI_FP_FN void fp_add(unsigned long long* p, unsigned long long v) {
#if defined(__HIPCC__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}

MI_FP_FN bool fp_finite(float x) { return x - x == 0.0f; }

// phase 0: clear the working set, fetch the lattice
MI_FP_FN void fp_phase_init(FpShared& s, const FpArgs& a, int b, int tid) {
    for (int e = tid; e < FP_ROW_MAX; e += FP_THREADS) {
        s.hist[e] = 0ull;
        s.g[e] = 0.f;
    }
    for (int z = tid; z < 101; z += FP_THREADS) {
        s.cnt[z] = 0;
        s.slot[z] = -1;
    }
    if (tid < 9) s.L[tid] = a.lattices[(size_t)b * 9 + tid];
    if (tid == 0) {
        s.bad_type = s.bad_coord = 0;
        s.status = MI_FP_OK;
        s.m = 0;
        s.V = s.norm = s.images = 0.f;
        s.reach[0] = s.reach[1] = s.reach[2] = 0;
    }
}

// phase 1: count the atoms of every species, look at every type and coordinate once
MI_FP_FN void fp_phase_scan(FpShared& s, const FpArgs& a, int b, int tid) {
    const int n0 = a.node_off[b], n = a.node_off[b + 1] - n0;
    for (int i = tid; i < n; i += FP_THREADS) {
        const int z = a.atom_types[n0 + i];
        if (z < 1 || z > 100) s.bad_type = 1;   // (every writer stores the same value)
        else fp_add(&s.cnt[z], 1);
        const float* x = a.frac + (size_t)(n0 + i) * 3;
        if (!(fp_finite(x[0]) && fp_finite(x[1]) && fp_finite(x[2]))) s.bad_coord = 1;
    }
}

MI_FP_FN float fp_cross_norm(const float* u, const float* v) {
    const float c0 = u[1] * v[2] - u[2] * v[1], c1 = u[2] * v[0] - u[0] * v[2], c2 = u[0] * v[1] - u[1] * v[0];
    return sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
}

// phase 2 (thread 0): the verdict -- species ranks and block table, volume, the reach of the translations from the perpendicular heights
MI_FP_FN void fp_phase_verdict(FpShared& s, const FpArgs& a, int b, int tid) {
    if (tid != 0) return;
    const int n = a.node_off[b + 1] - a.node_off[b];
    int m = 0;
    for (int z = 1; z <= 100; ++z)
        if (s.cnt[z] > 0) {
            if (m < MI_FP_MAX_SPECIES) {
                s.slot[z] = m;
                s.na[m] = s.cnt[z];
            }
            ++m;
        }
    s.m = m;
    const int mm = m < MI_FP_MAX_SPECIES ? m : MI_FP_MAX_SPECIES;
    int blk = 0;
    for (int p = 0; p < mm; ++p)
        for (int q = p; q < mm; ++q) {
            s.blk_a[blk] = p;
            s.blk_b[blk] = q;
            ++blk;
        }
    for (; blk < MI_FP_MAX_BLOCKS; ++blk) s.blk_a[blk] = s.blk_b[blk] = -1;

    const float* L = s.L;
    bool finite = !s.bad_coord;
    for (int k = 0; k < 9; ++k) finite = finite && fp_finite(L[k]);
    const float cn[3] = {fp_cross_norm(L + 3, L + 6), fp_cross_norm(L + 6, L), fp_cross_norm(L, L + 3)};
    const float c0 = L[4] * L[8] - L[5] * L[7], c1 = L[5] * L[6] - L[3] * L[8], c2 = L[3] * L[7] - L[4] * L[6];
    const float V = fabsf((L[0] * c0 + L[1] * c1) + L[2] * c2);
    finite = finite && fp_finite(V) && fp_finite(cn[0]) && fp_finite(cn[1]) && fp_finite(cn[2]);
    int status = MI_FP_OK;
    if (n <= 0 || s.bad_type) status = MI_FP_ATOMS;
    else if (!finite) status = MI_FP_NONFINITE;
    else if (!(V >= MI_FP_MIN_VOLUME)) status = MI_FP_VOLUME;
    else {
        s.V = V;
        const float rc = a.r_max + MI_FP_CUT * a.sigma;
        float images = 1.f;
        for (int ax = 0; ax < 3; ++ax) {
            // |t| <= rc / h + 1/2 with h = V / |b x c| (the wrapped difference lies in [-1/2, 1/2]); a hair generous against fp32 rounding
            const float x = (rc * cn[ax] / V) * 1.00001f + 0.5f;
            if (!(x <= (float)MI_FP_MAX_REACH)) {
                status = MI_FP_REACH;
                break;
            }
            s.reach[ax] = (int)ceilf(x);
            images *= (float)(2 * s.reach[ax] + 1);
        }
        if (status == MI_FP_OK) {
            s.images = images;
            if (m > MI_FP_MAX_SPECIES) status = MI_FP_SPECIES;
        }
    }
    s.status = status;
}

// phase 3: the histogram.  Work item = (i, j, t_a, t_b), strided over the block; the third translation is the inner loop.
MI_FP_FN void fp_phase_accumulate(FpShared& s, const FpArgs& a, int b, int tid) {
    if (s.status != MI_FP_OK) return;
    const int n0 = a.node_off[b], n = a.node_off[b + 1] - n0, nbins = a.nbins, m = s.m;
    const int ra = s.reach[0], rb = s.reach[1], rc_ = s.reach[2], wa = 2 * ra + 1, wb = 2 * rb + 1;
    const float cut = MI_FP_CUT * a.sigma, rc = a.r_max + cut, rc2 = rc * rc;
    const float D = a.r_max / (float)nbins, invD = (float)nbins / a.r_max, inv_s2 = 1.0f / (a.sigma * 1.41421356237309505f);
    const float* L = s.L;
    const int64_t total = (int64_t)n * n * wa * wb;
    for (int64_t w = tid; w < total; w += FP_THREADS) {
        const int tb = (int)(w % wb);
        int64_t r = w / wb;
        const int ta = (int)(r % wa);
        r /= wa;
        const int j = (int)(r % n), i = (int)(r / n);
        const int si = s.slot[a.atom_types[n0 + i]], sj = s.slot[a.atom_types[n0 + j]];
        if (si > sj) continue;                       // block (a <= b) takes the ordered pairs (i in A_a, j in A_b)
        const int blk = si * m - si * (si - 1) / 2 + (sj - si);
        const float* xi = a.frac + (size_t)(n0 + i) * 3;
        const float* xj = a.frac + (size_t)(n0 + j) * 3;
        float d[3];
        for (int c = 0; c < 3; ++c) {
            d[c] = xj[c] - xi[c];
            d[c] -= rintf(d[c]);
        }
        const float fa = d[0] + (float)(ta - ra), fb = d[1] + (float)(tb - rb);
        float base[3];
        for (int c = 0; c < 3; ++c) base[c] = (fa * L[c] + fb * L[3 + c]) + d[2] * L[6 + c];
        const bool self_ab = i == j && ta == ra && tb == rb;
        unsigned long long* h = s.hist + blk * nbins;
        for (int tc = -rc_; tc <= rc_; ++tc) {
            const float p0 = base[0] + (float)tc * L[6], p1 = base[1] + (float)tc * L[7], p2 = base[2] + (float)tc * L[8];
            const float s2 = (p0 * p0 + p1 * p1) + p2 * p2;
            if (!(s2 <= rc2) || (self_ab && tc == 0)) continue;
            const float R = sqrtf(s2);
            int k_lo = (int)floorf((R - cut) * invD), k_hi = (int)floorf((R + cut) * invD);
            k_lo = k_lo < 0 ? 0 : k_lo;
            k_hi = k_hi > nbins - 1 ? nbins - 1 : k_hi;
            if (k_lo > k_hi) continue;
            float e_prev = erff(((float)k_lo * D - R) * inv_s2);
            for (int k = k_lo; k <= k_hi; ++k) {
                const float e_next = erff(((float)(k + 1) * D - R) * inv_s2);
                float mass = 0.5f * (e_next - e_prev);
                e_prev = e_next;
                mass = mass > 0.f ? mass : 0.f;
                fp_add(&h[k], (unsigned long long)(mass * FP_SCALE));
            }
        }
    }
}

// phase 4: sqrt(w_ab) F_ab(k) of the thread's elements and the thread's share of the squared norm
MI_FP_FN void fp_phase_weigh(FpShared& s, const FpArgs& a, int b, int tid) {
    float acc = 0.f;
    if (s.status == MI_FP_OK) {
        const int n = a.node_off[b + 1] - a.node_off[b], nbins = a.nbins, m = s.m;
        const int row = (m * (m + 1) / 2) * nbins;
        const float D = a.r_max / (float)nbins;
        for (int e = tid; e < row; e += FP_THREADS) {
            const int blk = e / nbins, k = e % nbins, p = s.blk_a[blk], q = s.blk_b[blk];
            const float nab = (float)s.na[p] * (float)s.na[q];
            const float C = (float)((double)s.hist[e] * FP_INV_SCALE);
            const float Rk = ((float)k + 0.5f) * D;
            const float shell = (12.5663706143591730f * Rk * Rk * D) * nab / s.V;
            const float F = C / shell - 1.0f;
            const float wgt = (p < q ? 2.0f : 1.0f) * nab / ((float)n * (float)n);
            const float g = sqrtf(wgt) * F;
            s.g[e] = g;
            acc += g * g;
        }
    }
    s.red[tid] = acc;
}

// phase 5 (thread 0): the norm, summed in thread order, and the info row
MI_FP_FN void fp_phase_norm(FpShared& s, const FpArgs& a, int b, int tid) {
    if (tid != 0) return;
    if (s.status == MI_FP_OK) {
        double t = 0.0;
        for (int k = 0; k < FP_THREADS; ++k) t += (double)s.red[k];
        const float norm = (float)sqrt(t);
        if (fp_finite(norm) && norm > 0.f) s.norm = norm;
        else s.status = MI_FP_NONFINITE;
    }
    float* info = a.out_info + (size_t)b * 4;
    info[0] = (float)s.m;
    info[1] = (float)s.status;
    info[2] = s.status == MI_FP_OK ? s.norm : 0.f;
    info[3] = s.images;
}

// phase 6: the unit row (zeros for a flagged crystal and for the blocks past the crystal's own)
MI_FP_FN void fp_phase_store(FpShared& s, const FpArgs& a, int b, int tid) {
    const int len = MI_FP_MAX_BLOCKS * a.nbins;
    float* out = a.out_fp + (size_t)b * len;
    const bool ok = s.status == MI_FP_OK;
    const int row = ok ? (s.m * (s.m + 1) / 2) * a.nbins : 0;
    for (int e = tid; e < len; e += FP_THREADS) out[e] = e < row ? s.g[e] / s.norm : 0.f;
}

}  // namespace mi

#endif
