// The fingerprint-matching kernels' body (include/matinvent_hip_match.h), written as the phases between the barriers and the
// cross-lane exchanges so that the very same source also compiles for the host, where a stand-alone program runs every phase as a loop
// over the thread index (scripts/fp_match_host_check.cpp: bounds and guards under the host sanitizers).  Plain C++: the only device
// intrinsic, the lane exchange of the butterfly, stays in fp_match.hip; the host program exchanges through an array.
#ifndef MI_FP_MATCH_BODY_H
#define MI_FP_MATCH_BODY_H

#include <cmath>
#include <cstdint>

#include "../../include/matinvent_hip_match.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI_FPM_FN __host__ __device__ __forceinline__
#define MI_FPM_UNROLL _Pragma("unroll")
#else
#define MI_FPM_FN static inline
#define MI_FPM_UNROLL
#endif

namespace mi {

constexpr int FPM_THREADS = 256, FPM_WAVE = 64, FPM_WAVES = FPM_THREADS / FPM_WAVE;
constexpr int FPM_TQ = MI_FP_MATCH_TILE;     // query rows per tile
constexpr int FPM_CW = 4;                    // candidates a wave carries through one pass: FPM_CW x FPM_TQ = 32 sums, one per lane pair
constexpr int FPM_NV = FPM_CW * FPM_TQ;
constexpr int FPM_PASS = FPM_WAVES * FPM_CW; // candidates per block pass
constexpr int FPM_MAX_LEN = MI_FP_MAX_BLOCKS * MI_FP_MAX_BINS;
constexpr int FPM_UNWRITTEN = -1;             // every partial's status before the launch (the entry fills the array): an item that is rejected writes none
static_assert(FPM_NV * 2 == FPM_WAVE, "the halving butterfly leaves one sum per lane pair");

struct FpmArgs {
    mi_fp_match_args a;
    float* part_dist;   // [n_partials]
    int* part_idx;
    int* part_cnt;
    int* part_status;
};

// one work item's bookkeeping: LDS on the device (the tile of query rows is a separate, dynamically sized array), an object on the host
struct FpmShared {
    int ok, g, q0, nq, c0, c1, len, nq_g, nc_g, part_base, pairs;
    long long pair_base;
    float w_dist[FPM_WAVES][FPM_NV];
    int w_idx[FPM_WAVES][FPM_NV], w_cnt[FPM_WAVES][FPM_NV], w_status[FPM_WAVES];
};

// what a lane carries across the passes of an item
struct FpmLane {
    float v[FPM_NV];                    // v[k * FPM_TQ + q]: this lane's share of candidate k . query q
    int row;                            // bank row of the candidate whose sums end in this lane (slot lane / 16 of the pass); -1: none or skipped
    float best;
    int best_i, cnt, skipped;
};

MI_FPM_FN int fpm_round4(int n) { return (n + 3) / 4 * 4; }

// four floats at a 16-byte aligned address: one 16-byte access on the device
MI_FPM_FN void fpm_load4(const float* p, float* x) {
#if defined(__HIPCC__)
    const float4 t = *reinterpret_cast<const float4*>(p);
    x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
#else
    x[0] = p[0], x[1] = p[1], x[2] = p[2], x[3] = p[3];
#endif
}

MI_FPM_FN void fpm_store4(float* p, const float* x) {
#if defined(__HIPCC__)
    *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
#else
    p[0] = x[0], p[1] = x[1], p[2] = x[2], p[3] = x[3];
#endif
}

// ---- the plan (host) --------------------------------------------------------------------------------------------------------------------
inline int64_t fpm_plan_count(const int* q_off, const int* c_off, int G, int chunk, int64_t* parts) {
    int64_t items = 0, np = 0;
    for (int g = 0; g < G; ++g) {
        const int64_t nq = q_off[g + 1] - q_off[g], nc = c_off[g + 1] - c_off[g];
        const int64_t tiles = (nq + FPM_TQ - 1) / FPM_TQ, chunks = (nc + chunk - 1) / chunk;
        items += tiles * chunks;
        np += tiles * chunks * FPM_TQ;
    }
    *parts = np;
    return items;
}

// returns the chunk used, or -1
inline int fpm_plan(const int* q_off, const int* c_off, int G, int chunk, int* items, int* part_off, int64_t* n_items, int64_t* n_parts) {
    if (!q_off || !c_off || !n_items || !n_parts || G < 0 || (items == nullptr) != (part_off == nullptr)) return -1;
    if (G > 0 && (q_off[0] < 0 || c_off[0] < 0)) return -1;
    for (int g = 0; g < G; ++g)
        if (q_off[g + 1] < q_off[g] || c_off[g + 1] < c_off[g]) return -1;
    int64_t ni, np;
    if (chunk <= 0) {
        chunk = 1024;
        while ((ni = fpm_plan_count(q_off, c_off, G, chunk, &np)) < 2048 && chunk > 32) chunk /= 2;
    } else {
        chunk = (chunk + FPM_PASS - 1) / FPM_PASS * FPM_PASS;
    }
    ni = fpm_plan_count(q_off, c_off, G, chunk, &np);
    if (ni * MI_FP_MATCH_ITEM_INTS > INT32_MAX || np > INT32_MAX) return -1;
    *n_items = ni;
    *n_parts = np;
    if (!items) return chunk;
    int64_t it = 0, part = 0;
    for (int g = 0; g < G; ++g) {
        part_off[g] = (int)part;
        for (int q = q_off[g]; q < q_off[g + 1]; q += FPM_TQ)
            for (int c = c_off[g]; c < c_off[g + 1]; c += chunk) {
                int* e = items + it * MI_FP_MATCH_ITEM_INTS;
                e[0] = g;
                e[1] = q;
                e[2] = c;
                e[3] = c + chunk < c_off[g + 1] ? c + chunk : c_off[g + 1];
                e[4] = (int)part;
                part += FPM_TQ;
                ++it;
            }
    }
    part_off[G] = (int)part;
    return chunk;
}

// ---- phase 0 (thread 0): decode the item and check that it lies inside its group and the arrays ---------------------------------------------
MI_FPM_FN void fpm_phase_item(FpmShared& s, const FpmArgs& A, int item, int tid) {
    if (tid != 0) return;
    const mi_fp_match_args& a = A.a;
    const int* e = a.items + (size_t)item * MI_FP_MATCH_ITEM_INTS;
    const int g = e[0], q0 = e[1], c0 = e[2], c1 = e[3], pb = e[4];
    s.ok = 0;
    s.pairs = 0;
    if (g < 0 || g >= a.G) return;
    const int qa = a.grp_q_off[g], qb = a.grp_q_off[g + 1], ca = a.grp_c_off[g], cb = a.grp_c_off[g + 1], ncols = a.grp_ncols[g];
    if (qa < 0 || qb > a.nnz_q || qa > qb || ca < 0 || cb > a.nnz_c || ca > cb) return;
    if (q0 < qa || q0 >= qb || c0 < ca || c0 >= c1 || c1 > cb) return;
    if (pb < 0 || pb > a.n_partials - FPM_TQ) return;
    if (ncols < 1 || ncols > FPM_MAX_LEN) return;
    const int len = fpm_round4(ncols);
    if (len > a.row_stride || len > fpm_round4(a.max_ncols)) return;
    s.g = g;
    s.q0 = q0;
    s.nq = qb - q0 < FPM_TQ ? qb - q0 : FPM_TQ;
    s.c0 = c0;
    s.c1 = c1;
    s.len = len;
    s.nq_g = qb - qa;
    s.nc_g = cb - ca;
    s.part_base = pb;
    if (a.pair_dist && a.pair_off) {
        const long long base = a.pair_off[g];
        if (base >= 0 && base + (long long)s.nq_g * s.nc_g <= a.pair_floats) {
            s.pairs = 1;
            s.pair_base = base + (long long)(q0 - qa) * s.nc_g + (c0 - ca);   // of (tile slot 0, the item's first candidate)
        }
    }
    s.ok = 1;
}

// ---- phase 1: the tile's query rows into LDS, 16 bytes per thread and step; absent rows are zero ----------------------------------------------
MI_FPM_FN void fpm_phase_stage(FpmShared& s, const FpmArgs& A, float* tile, int tid) {
    if (!s.ok) return;
    const mi_fp_match_args& a = A.a;
    const int len4 = s.len / 4;
    for (int e = tid; e < FPM_TQ * len4; e += FPM_THREADS) {
        const int q = e / len4, c4 = e % len4;
        int row = -1;
        if (q < s.nq) {
            row = a.q_idx[s.q0 + q];
            if (row < 0 || row >= a.Q) row = -1;
        }
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (row >= 0) fpm_load4(a.query + (size_t)row * a.row_stride + 4 * c4, x);
        fpm_store4(tile + (size_t)q * s.len + 4 * c4, x);
    }
}

MI_FPM_FN void fpm_lane_init(FpmLane& r) {
    r.best = INFINITY;
    r.best_i = -1;
    r.cnt = 0;
    r.skipped = 0;
}

// ---- a pass, step 1: the wave's FPM_CW candidates against the tile.  Lane l owns the columns 4 (l + 64 i) + k; i, then k, ascending ------------
MI_FPM_FN void fpm_pass_accumulate(const FpmShared& s, const FpmArgs& A, const float* tile, int tid, int pass, FpmLane& r) {
    const mi_fp_match_args& a = A.a;
    const int wave = tid / FPM_WAVE, lane = tid % FPM_WAVE, len = s.len;
    long long coff[FPM_CW];   // element offset of the row in the bank; -1: none
    MI_FPM_UNROLL
    for (int k = 0; k < FPM_CW; ++k) {
        const int pos = s.c0 + (pass * FPM_WAVES + wave) * FPM_CW + k;
        int row = -1;
        coff[k] = -1;
        if (pos < s.c1) {
            row = a.c_idx[pos];
            bool good = row >= 0 && row < a.M;
            if (good) {
                const long long st = a.bank_start[row];
                good = a.bank_len[row] == len && st >= 0 && (st & 3) == 0 && st + len <= a.bank_floats;
                if (good) coff[k] = st;
            }
            if (!good) {
                row = -1;
                r.skipped = 1;
            }
        }
        if (k == lane / (2 * FPM_TQ)) r.row = row;
    }
    MI_FPM_UNROLL
    for (int j = 0; j < FPM_NV; ++j) r.v[j] = 0.f;
    for (int col = 4 * lane; col < len; col += 4 * FPM_WAVE) {
        float c[FPM_CW][4];
        MI_FPM_UNROLL
        for (int k = 0; k < FPM_CW; ++k) {
            if (coff[k] >= 0) {
                fpm_load4(a.bank + coff[k] + col, c[k]);
            } else {
                c[k][0] = c[k][1] = c[k][2] = c[k][3] = 0.f;
            }
        }
        MI_FPM_UNROLL
        for (int q = 0; q < FPM_TQ; ++q) {
            float u[4];
            fpm_load4(tile + (size_t)q * len + col, u);
            const float u0 = u[0], u1 = u[1], u2 = u[2], u3 = u[3];
            MI_FPM_UNROLL
            for (int k = 0; k < FPM_CW; ++k) {
                float t = r.v[k * FPM_TQ + q];
                t = fmaf(c[k][0], u0, t);
                t = fmaf(c[k][1], u1, t);
                t = fmaf(c[k][2], u2, t);
                t = fmaf(c[k][3], u3, t);
                r.v[k * FPM_TQ + q] = t;
            }
        }
    }
}

// ---- a pass, step 2: one level of the butterfly with the partner lane (lane ^ mask), on `half` sums.  Before the level a lane holds
// 2 * half sums; it keeps the lower half if its `mask` bit is clear, the upper half if set, hands the other half to its partner and adds
// what the partner hands over.  For every sum this is the addition (lane l) + (lane l ^ mask): levels 32, 16, 8, 4, 2 leave lane l
// with sum number l / 2 over the lanes of its parity, and the last level (half = 0: mask 1, nothing to split) adds the two parities. ---------
MI_FPM_FN void fpm_level_send(const FpmLane& r, int lane, int mask, int half, float* send) {
    const bool upper = (lane & mask) != 0;
    if (half == 0) {
        send[0] = r.v[0];
        return;
    }
    MI_FPM_UNROLL
    for (int j = 0; j < half; ++j) {
        const float lo = r.v[j], hi = r.v[j + half];   // (values, not an lvalue choice: the sums stay in registers)
        send[j] = upper ? lo : hi;
    }
}

MI_FPM_FN void fpm_level_add(FpmLane& r, int lane, int mask, int half, const float* recv) {
    const bool upper = (lane & mask) != 0;
    if (half == 0) {
        r.v[0] = r.v[0] + recv[0];
        return;
    }
    MI_FPM_UNROLL
    for (int j = 0; j < half; ++j) {
        const float lo = r.v[j], hi = r.v[j + half];
        r.v[j] = (upper ? hi : lo) + recv[j];
    }
}

// ---- a pass, step 3: lane l holds the dot product of (candidate (l / 2) / FPM_TQ, query (l / 2) % FPM_TQ); the even lanes keep score ------------
MI_FPM_FN void fpm_pass_update(const FpmShared& s, const FpmArgs& A, int tid, int pass, FpmLane& r) {
    const mi_fp_match_args& a = A.a;
    const int wave = tid / FPM_WAVE, lane = tid % FPM_WAVE;
    if (lane & 1) return;
    const int j = lane / 2, k = j / FPM_TQ, q = j % FPM_TQ;
    const int row = r.row;
    if (row < 0 || q >= s.nq) return;
    const float d = 0.5f * (1.0f - r.v[0]);
    if (d < r.best || (d == r.best && row < r.best_i)) {
        r.best = d;
        r.best_i = row;
    }
    if (d <= a.tol) ++r.cnt;
    if (s.pairs) {
        const int cpos = (pass * FPM_WAVES + wave) * FPM_CW + k;   // relative to the item's first candidate
        a.pair_dist[s.pair_base + (long long)q * s.nc_g + cpos] = d;
    }
}

// ---- phase 3: every wave's scores to LDS ---------------------------------------------------------------------------------------------------
MI_FPM_FN void fpm_phase_wave_out(FpmShared& s, int tid, const FpmLane& r) {
    const int wave = tid / FPM_WAVE, lane = tid % FPM_WAVE;
    if (lane == 0) s.w_status[wave] = 0;
    if (!(lane & 1)) {
        s.w_dist[wave][lane / 2] = r.best;
        s.w_idx[wave][lane / 2] = r.best_i;
        s.w_cnt[wave][lane / 2] = r.cnt;
    }
}

// (every lane of a wave saw the same candidates: any one of them may report the skip; a separate phase so that the clearing store is ordered)
MI_FPM_FN void fpm_phase_wave_status(FpmShared& s, int tid, const FpmLane& r) {
    if (tid % FPM_WAVE == 1 && r.skipped) s.w_status[tid / FPM_WAVE] = 1;
}

MI_FPM_FN void fpm_fold(float d, int i, float& best, int& best_i) {
    if (i >= 0 && (best_i < 0 || d < best || (d == best && i < best_i))) {
        best = d;
        best_i = i;
    }
}

// ---- phase 4 (threads 0 .. FPM_TQ - 1): the item's partial of one query, waves and candidate slots in a fixed order -------------------------------
MI_FPM_FN void fpm_phase_partial(const FpmShared& s, const FpmArgs& A, int tid) {
    if (!s.ok || tid >= FPM_TQ) return;
    float best = INFINITY;
    int best_i = -1, cnt = 0, st = 0;
    for (int w = 0; w < FPM_WAVES; ++w) {
        st |= s.w_status[w];
        for (int k = 0; k < FPM_CW; ++k) {
            fpm_fold(s.w_dist[w][k * FPM_TQ + tid], s.w_idx[w][k * FPM_TQ + tid], best, best_i);
            cnt += s.w_cnt[w][k * FPM_TQ + tid];
        }
    }
    const int p = s.part_base + tid;
    A.part_dist[p] = best;
    A.part_idx[p] = best_i;
    A.part_cnt[p] = cnt;
    A.part_status[p] = st;
}

// ---- the second kernel: query position p folds its partials in chunk order ------------------------------------------------------------------
MI_FPM_FN void fpm_reduce_query(const FpmArgs& A, int p) {
    const mi_fp_match_args& a = A.a;
    if (p < 0 || p >= a.nnz_q) return;
    int lo = 0, hi = a.G;                      // the group g with grp_q_off[g] <= p < grp_q_off[g + 1]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (a.grp_q_off[mid] <= p) lo = mid;
        else hi = mid;
    }
    const int g = lo, qa = a.grp_q_off[g], qb = a.grp_q_off[g + 1];
    if (p < qa || p >= qb) return;
    const int row = a.q_idx[p];
    if (row < 0 || row >= a.Q) return;
    const int j = p - qa, tiles = (qb - qa + FPM_TQ - 1) / FPM_TQ, pa = a.grp_part_off[g], pb = a.grp_part_off[g + 1];
    const int chunks = pb > pa ? (pb - pa) / (FPM_TQ * tiles) : 0;
    float best = INFINITY;
    int best_i = -1, cnt = 0, st = 0;
    for (int k = 0; k < chunks; ++k) {
        const long long e = (long long)pa + ((long long)(j / FPM_TQ) * chunks + k) * FPM_TQ + j % FPM_TQ;
        if (e < 0 || e >= a.n_partials || A.part_status[e] == FPM_UNWRITTEN) {   // the item of this chunk was rejected (phase 0): skipped, and said so
            st = 1;
            continue;
        }
        fpm_fold(A.part_dist[e], A.part_idx[e], best, best_i);
        cnt += A.part_cnt[e];
        st |= A.part_status[e];
    }
    a.best_dist[row] = best;
    a.best_idx[row] = best_i;
    a.n_within[row] = cnt;
    a.status[row] = st;
}

}  // namespace mi

#endif
