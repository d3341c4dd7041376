// The structure matcher (include/matinvent_hip_smatch.h).  Launches of this unit, no atomics, no scratch, no matrix pipe:
//   sm_prepare_kernel       one wave per crystal, a lane per atom: the guard, the reduced and scaled cell (every lane, redundantly), the
//                           stable sort by species as a rank per lane, the block table and the rarest species;
//   sm_match_kernel<NMAX>   one 256-thread workgroup per pair: the lattice maps by ordered compaction (ballot, wave counts in LDS) of the
//                           box points and of the candidate triples into LDS; then the four waves stride over the (map, translation)
//                           items, a lane per column: the cost rows of a species block in the wave's LDS tile, the augmenting-path
//                           search with (value, column) xor butterflies, the RMS about the mean; the waves' (rms, item) pairs fold in a
//                           fixed order and wave 0 re-evaluates the best item for the permutation.  NMAX = 32 and 64 differ in the tile's
//                           size only.
// csrc/sm_lattice.h and csrc/sm_assign.h hold every formula, host and device.

#include <mutex>

#include "../../include/matinvent_hip_smatch.h"
#include "common.h"
#include "sm_assign.h"

namespace mi {

static_assert(SM_MAX_ATOMS == MI_SM_MAX_ATOMS && SM_MAX_SPECIES == MI_SM_MAX_SPECIES && SM_MAX_MAPS == MI_SM_MAX_MAPS && SM_MAX_CAND == MI_SM_MAX_CAND &&
                  SM_BOX_CAP == MI_SM_BOX_POINTS,
              "sizes");
static_assert(SM_PREP_OK == MI_SM_PREP_OK && SM_PREP_BAD_INPUT == MI_SM_PREP_BAD_INPUT && SM_PREP_TOO_MANY_ATOMS == MI_SM_PREP_TOO_MANY_ATOMS &&
                  SM_PREP_TOO_MANY_SPECIES == MI_SM_PREP_TOO_MANY_SPECIES && SM_PREP_DEGENERATE_CELL == MI_SM_PREP_DEGENERATE_CELL &&
                  SM_PREP_REDUCE_CAP == MI_SM_PREP_REDUCE_CAP,
              "prepare codes");
static_assert(SM_OK == MI_SM_OK && SM_NO_LATTICE == MI_SM_NO_LATTICE && SM_BOX_CAP_HIT == MI_SM_BOX_CAP && SM_MAP_CAP_HIT == MI_SM_MAP_CAP &&
                  SM_SPECIES_MISMATCH == MI_SM_SPECIES_MISMATCH && SM_BAD_PAIR == MI_SM_BAD_PAIR && SM_NOT_PREPARED == MI_SM_NOT_PREPARED,
              "pair codes");
static_assert(SM_MIN_VOLUME == MI_SM_MIN_VOLUME, "volume floor");

constexpr int SM_WAVES = SM_THREADS / 64;
constexpr int SM_NO_COL = 0x7fffffff;

struct SmPrepArgs {
    const int* types;
    const float* frac;
    const float* lat;
    mi_sm_prepared o;
};

__device__ __forceinline__ int sm_lanes_below(uint64_t mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

// LDS written by other lanes of this wave is read next
__device__ __forceinline__ void sm_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(64) void sm_prepare_kernel(SmPrepArgs A) {
    __shared__ int s_off[SM_MAX_SPECIES + 1];
    const int b = blockIdx.x, lane = threadIdx.x;
    int* info = A.o.info + (size_t)b * 4;
    const int n0 = A.o.offsets[b], n1 = A.o.offsets[b + 1];
    if (!(n0 >= 0 && n0 <= n1 && n1 <= A.o.N)) {   // (uniform) nothing is read through these offsets
        if (lane < 4) info[lane] = lane == 3 ? SM_PREP_BAD_INPUT : 0;
        return;
    }
    const int n = n1 - n0;
    if (n < 1 || n > SM_MAX_ATOMS) {
        if (lane < 4) info[lane] = lane == 0 ? n : (lane == 3 ? (n < 1 ? SM_PREP_BAD_INPUT : SM_PREP_TOO_MANY_ATOMS) : 0);
        return;
    }
    const float* lat = A.lat + (size_t)b * 9;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 9; ++i) bad = bad || !sm_finite((double)lat[i]);
    int z = 0;
    if (lane < n) {
        z = A.types[n0 + lane];
        bad = bad || z < 1 || z > SM_MAX_Z;
#pragma unroll
        for (int c = 0; c < 3; ++c) bad = bad || !sm_finite((double)A.frac[(size_t)(n0 + lane) * 3 + c]);
    }
    if (__any(bad)) {
        if (lane < 4) info[lane] = lane == 0 ? n : (lane == 3 ? SM_PREP_BAD_INPUT : 0);
        return;
    }
    int rank = 0, sidx = 0, cnt = 0;
    bool first = false;
    if (lane < n) sm_sort_lane(A.types + n0, n, lane, &rank, &first, &sidx, &cnt);
    const int nspec = __popcll(__ballot(first));
    if (nspec > SM_MAX_SPECIES) {
        if (lane < 4) info[lane] = lane == 0 ? n : (lane == 3 ? SM_PREP_TOO_MANY_SPECIES : 0);
        return;
    }
    int T[9];
    double Ls[9], inv[9];
    const int st = sm_prepare_cell(lat, n, T, Ls, inv);   // (uniform)
    if (st != SM_PREP_OK) {
        if (lane < 4) info[lane] = lane == 0 ? n : (lane == 3 ? st : 0);
        return;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i)
        if (lane == i) A.o.lat[(size_t)b * 9 + i] = Ls[i], A.o.inv[(size_t)b * 9 + i] = inv[i];
    if (lane < n) {
        double f[3];
        sm_reduced_frac(A.frac + (size_t)(n0 + lane) * 3, T, f);
        const size_t d = (size_t)(n0 + rank);
        A.o.frac[d * 3] = f[0], A.o.frac[d * 3 + 1] = f[1], A.o.frac[d * 3 + 2] = f[2];
        A.o.types[d] = z, A.o.perm[d] = lane;
        if (first) A.o.spec_Z[(size_t)b * SM_MAX_SPECIES + sidx] = z, A.o.spec_off[(size_t)b * (SM_MAX_SPECIES + 1) + sidx] = rank, s_off[sidx] = rank;
    }
    if (lane >= nspec && lane < SM_MAX_SPECIES) A.o.spec_Z[(size_t)b * SM_MAX_SPECIES + lane] = 0;
    if (lane >= nspec && lane <= SM_MAX_SPECIES) A.o.spec_off[(size_t)b * (SM_MAX_SPECIES + 1) + lane] = n, s_off[lane] = n;
    __syncthreads();
    if (lane == 0) info[0] = n, info[1] = nspec, info[2] = sm_rarest(s_off, nspec), info[3] = SM_PREP_OK;
}

// ---- the match kernel's LDS --------------------------------------------------------------------------------------------------------------------
// [maps 256 x 9 int][L1, L2 18 double][f1, f2 NMAX x 3 double each][per wave: tile NMAX^2, f2' NMAX x 3, u NMAX x 3, d2 NMAX double,
// col NMAX int]; the candidate lists (3 axes x SM_MAX_CAND x (v[3], len double; k[3] int)) lie over the tiles, which are dead until the
// map list is complete.
template <int NMAX>
struct SmLds {
    static constexpr size_t maps = 0;
    static constexpr size_t cell = maps + sizeof(int) * SM_MAX_MAPS * 9;
    static constexpr size_t f1 = cell + sizeof(double) * 18;
    static constexpr size_t f2 = f1 + sizeof(double) * NMAX * 3;
    static constexpr size_t waves = f2 + sizeof(double) * NMAX * 3;
    static constexpr size_t tile = 0, f2p = tile + sizeof(double) * NMAX * NMAX, u = f2p + sizeof(double) * NMAX * 3, d2 = u + sizeof(double) * NMAX * 3,
                            col = d2 + sizeof(double) * NMAX, wave_bytes = col + sizeof(int) * NMAX;
    static constexpr size_t bytes = waves + SM_WAVES * wave_bytes;
    static constexpr size_t cand_v = waves, cand_len = cand_v + sizeof(double) * 3 * SM_MAX_CAND * 3, cand_k = cand_len + sizeof(double) * 3 * SM_MAX_CAND,
                            cand_end = cand_k + sizeof(int) * 3 * SM_MAX_CAND * 3;
    static_assert(cand_end <= bytes, "the candidate lists fit over the tiles");
    static_assert(bytes <= 160 * 1024, "gfx950: 160 KB of LDS per workgroup");
};

struct SmWave {
    double* tile;
    double* f2p;
    double* u;
    double* d2;
    int* col;
};

// The assignment of one species block, a lane per column (and per row): sm_assign_serial's steps.  tile [nb][nb]; returns this lane's
// column (lane < nb) or SM_NO_COL when a cost was not a number.
__device__ __forceinline__ int sm_wave_assign(const double* tile, int nb, int lane) {
    double u = 0.0, v = 0.0;
    int row4col = -1, col4row = -1, path = -1;
    for (int cur = 0; cur < nb; ++cur) {
        double shortest = sm_inf(), min_val = 0.0;
        bool SR = false, SC = lane >= nb;
        int i = cur, sink = -1;
        while (sink < 0) {   // (uniform)
            if (lane == i) SR = true;
            const double ui = __shfl(u, i, 64);
            if (!SC) {
                const double r = sm_reduced(min_val, tile[i * nb + lane], ui, v);
                if (r < shortest) shortest = r, path = i;
            }
            double bv = SC ? sm_inf() : shortest;
            int bj = SC ? SM_NO_COL : lane;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double ov = __shfl_xor(bv, m, 64);
                const int oj = __shfl_xor(bj, m, 64);
                if (sm_better(ov, oj, bv, bj)) bv = ov, bj = oj;
            }
            if (bj >= nb || !(bv < sm_inf())) return SM_NO_COL;   // (uniform) no column within reach: a cost that is not a finite number
            min_val = bv;
            if (lane == bj) SC = true;
            const int r4 = __shfl(row4col, bj, 64);
            if (r4 < 0) sink = bj;
            else i = r4;
        }
        const double sc = __shfl(shortest, col4row < 0 ? 0 : col4row, 64);
        if (lane == cur) u = u + min_val;
        else if (SR) u = u + (min_val - sc);
        if (SC && lane < nb) v = v - (min_val - shortest);
        int j = sink;
        for (int step = 0; step <= nb; ++step) {   // (uniform) the augmenting path has at most nb edges
            const int r = __shfl(path, j, 64);
            if (lane == j) row4col = r;
            const int old = __shfl(col4row, r, 64);
            if (lane == r) col4row = j;
            j = old;
            if (r == cur) break;
        }
    }
    return lane < nb ? col4row : SM_NO_COL;
}

struct SmPair {
    const double* f1;    // LDS: the query's sorted coordinates
    const double* f2;    // LDS: the candidate's
    const double* L1;    // LDS
    const double* L2;    // LDS
    const int* maps;     // LDS
    const int* spec_off; // global: the block table (of the query; the candidate's is equal)
    int n, nspec, r0, ntrans;
};

// One (map, translation) item on one wave: rms and max_dist; W.col holds the assignment (sorted candidate index per sorted query atom).
__device__ __forceinline__ bool sm_wave_item(const SmPair& P, const SmWave& W, int item, int lane, double* rms, double* max_dist) {
    const int m = item / P.ntrans, j = item - m * P.ntrans;
    int M[9], Mi[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) M[i] = P.maps[m * 9 + i];
    sm_map_inverse(M, Mi);
    double G[9];
    sm_metric(P.L1, P.L2, M, G);
    sm_wave_sync();   // the previous item's reads of W are done
    if (lane < P.n) {
        double f[3];
        sm_map_frac(P.f2 + 3 * lane, Mi, f);
        W.f2p[3 * lane] = f[0], W.f2p[3 * lane + 1] = f[1], W.f2p[3 * lane + 2] = f[2];
    }
    sm_wave_sync();
    double t[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = P.f1[3 * (P.r0 + j) + c] - W.f2p[3 * P.r0 + c];
    bool ok = true;
    for (int s = 0; s < P.nspec; ++s) {   // (uniform)
        const int b0 = P.spec_off[s], nb = P.spec_off[s + 1] - b0;
        if (lane < nb) {
            double f2b[3] = {W.f2p[3 * (b0 + lane)], W.f2p[3 * (b0 + lane) + 1], W.f2p[3 * (b0 + lane) + 2]};
            for (int a = 0; a < nb; ++a) {
                double u[3];
                W.tile[a * nb + lane] = sm_pair_cost(G, P.f1 + 3 * (b0 + a), f2b, t, u);
            }
        }
        sm_wave_sync();
        const int col = sm_wave_assign(W.tile, nb, lane);
        ok = ok && __all(lane >= nb || col != SM_NO_COL);
        if (lane < nb && col != SM_NO_COL) {
            double u[3];
            sm_pair_cost(G, P.f1 + 3 * (b0 + lane), W.f2p + 3 * (b0 + col), t, u);
            W.u[3 * (b0 + lane)] = u[0], W.u[3 * (b0 + lane) + 1] = u[1], W.u[3 * (b0 + lane) + 2] = u[2];
            W.col[b0 + lane] = b0 + col;
        }
        sm_wave_sync();   // the tile is rewritten by the next block
    }
    if (!ok) {   // (uniform)
        *rms = sm_inf(), *max_dist = sm_inf();
        return false;
    }
    double mean[3];
    sm_mean(W.u, P.n, mean);
    if (lane < P.n) W.d2[lane] = sm_centred(G, W.u + 3 * lane, mean);
    sm_wave_sync();
    sm_rms(W.d2, P.n, rms, max_dist);
    return true;
}

__device__ __forceinline__ void sm_fail(const mi_sm_match_args& a, int p, int tid, int status, int n_maps) {
    if (tid == 0) {
        a.rms[p] = sm_inf(), a.max_dist[p] = sm_inf(), a.best_trans[p] = -1, a.n_maps[p] = n_maps, a.n_items[p] = 0, a.status[p] = status;
    }
    if (tid < 9) a.best_map[(size_t)p * 9 + tid] = 0;
    if (a.perm && tid < SM_MAX_ATOMS) a.perm[(size_t)p * SM_MAX_ATOMS + tid] = -1;
}

template <int NMAX>
__global__ __launch_bounds__(SM_THREADS) void sm_match_kernel(mi_sm_match_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_lds[];
    __shared__ int s_count[2][3][SM_WAVES];
    __shared__ double s_best_v[SM_WAVES], s_best_m[SM_WAVES];
    __shared__ int s_best_i[SM_WAVES];
    using Lds = SmLds<NMAX>;
    const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int q = a.pair_q[p], c = a.pair_c[p];
    // ---- the guard and the tile class (uniform)
    int status = SM_OK, n = 0;
    if (q < 0 || q >= a.a.B || c < 0 || c >= a.b.B) status = SM_BAD_PAIR;
    const int* ia = a.a.info + (size_t)(status == SM_OK ? q : 0) * 4;
    const int* ib = a.b.info + (size_t)(status == SM_OK ? c : 0) * 4;
    if (status == SM_OK && (ia[3] != SM_PREP_OK || ib[3] != SM_PREP_OK)) status = SM_NOT_PREPARED;
    if (status == SM_OK) {
        n = ia[0];
        const int* za = a.a.spec_Z + (size_t)q * SM_MAX_SPECIES;
        const int* zb = a.b.spec_Z + (size_t)c * SM_MAX_SPECIES;
        const int* oa = a.a.spec_off + (size_t)q * (SM_MAX_SPECIES + 1);
        const int* ob = a.b.spec_off + (size_t)c * (SM_MAX_SPECIES + 1);
        bool same = ia[0] == ib[0] && ia[1] == ib[1];
        for (int s = 0; s < SM_MAX_SPECIES; ++s) same = same && za[s] == zb[s] && oa[s] == ob[s];
        if (!same) status = SM_SPECIES_MISMATCH;
    }
    const int cls = (status == SM_OK && (n > MI_SM_SMALL_ATOMS || a.large_tile)) ? 64 : 32;
    if (cls != NMAX) return;   // (uniform) the other launch owns this pair
    if (status != SM_OK) {
        sm_fail(a, p, tid, status, 0);
        return;
    }
    int* maps = reinterpret_cast<int*>(sm_lds + Lds::maps);
    double* cell = reinterpret_cast<double*>(sm_lds + Lds::cell);
    double* f1 = reinterpret_cast<double*>(sm_lds + Lds::f1);
    double* f2 = reinterpret_cast<double*>(sm_lds + Lds::f2);
    double* cand_v = reinterpret_cast<double*>(sm_lds + Lds::cand_v);
    double* cand_len = reinterpret_cast<double*>(sm_lds + Lds::cand_len);
    int* cand_k = reinterpret_cast<int*>(sm_lds + Lds::cand_k);
    const int n0a = a.a.offsets[q], n0b = a.b.offsets[c];
    if (tid < 9) cell[tid] = a.a.lat[(size_t)q * 9 + tid], cell[9 + tid] = a.b.lat[(size_t)c * 9 + tid];
    for (int i = tid; i < 3 * n; i += SM_THREADS) f1[i] = a.a.frac[(size_t)n0a * 3 + i], f2[i] = a.b.frac[(size_t)n0b * 3 + i];
    __syncthreads();
    const double* L1 = cell;
    const double* L2 = cell + 9;
    // ---- the candidate vectors of the three axes, in lexicographic order of k
    SmTarget tg;
    sm_target(L1, &tg);
    int bound[3];
    const int pts = sm_box(tg, a.b.inv + (size_t)c * 9, a.ltol, bound);
    if (pts < 0) {
        sm_fail(a, p, tid, SM_BOX_CAP_HIT, 0);
        return;
    }
    int ncand[3] = {0, 0, 0};
    int round = 0;
    for (int base = 0; base < pts; base += SM_THREADS, ++round) {
        const int pt = base + tid;
        int k[3] = {0, 0, 0};
        double v[3] = {0.0, 0.0, 0.0}, len = 0.0;
        if (pt < pts) sm_box_point(pt, bound, L2, k, v, &len);
        uint64_t mask[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            mask[ax] = __ballot(pt < pts && sm_length_ok(len, tg.len[ax], a.ltol));
            if (lane == 0) s_count[round & 1][ax][wave] = __popcll(mask[ax]);
        }
        __syncthreads();
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            int before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < SM_WAVES; ++w) {
                const int cw = s_count[round & 1][ax][w];
                before += w < wave ? cw : 0, total += cw;
            }
            const int at = ncand[ax] + before + sm_lanes_below(mask[ax], lane);
            if (((mask[ax] >> lane) & 1ull) && at < SM_MAX_CAND) {
                const int e = ax * SM_MAX_CAND + at;
                cand_v[3 * e] = v[0], cand_v[3 * e + 1] = v[1], cand_v[3 * e + 2] = v[2], cand_len[e] = len;
                cand_k[3 * e] = k[0], cand_k[3 * e + 1] = k[1], cand_k[3 * e + 2] = k[2];
            }
            ncand[ax] += total;
        }
    }
    __syncthreads();
    if (ncand[0] > SM_MAX_CAND || ncand[1] > SM_MAX_CAND || ncand[2] > SM_MAX_CAND) {
        sm_fail(a, p, tid, SM_BOX_CAP_HIT, 0);
        return;
    }
    // ---- the maps: candidate triples in nested ascending order
    const int64_t triples = (int64_t)ncand[0] * ncand[1] * ncand[2];
    int nmaps = 0;
    for (int64_t base = 0; base < triples && nmaps <= SM_MAX_MAPS; base += SM_THREADS, ++round) {
        const int64_t t = base + tid;
        bool ok = false;
        int e0 = 0, e1 = 0, e2 = 0;
        if (t < triples) {
            e0 = (int)(t / ((int64_t)ncand[1] * ncand[2]));
            e1 = SM_MAX_CAND + (int)((t / ncand[2]) % ncand[1]);
            e2 = 2 * SM_MAX_CAND + (int)(t % ncand[2]);
            ok = sm_triple_ok(tg, cand_v + 3 * e0, cand_len[e0], cand_k + 3 * e0, cand_v + 3 * e1, cand_len[e1], cand_k + 3 * e1, cand_v + 3 * e2, cand_len[e2],
                              cand_k + 3 * e2, a.cos_tol);
        }
        const uint64_t mask = __ballot(ok);
        if (lane == 0) s_count[round & 1][0][wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SM_WAVES; ++w) {
            const int cw = s_count[round & 1][0][w];
            before += w < wave ? cw : 0, total += cw;
        }
        const int at = nmaps + before + sm_lanes_below(mask, lane);
        if (ok && at < SM_MAX_MAPS) {
#pragma unroll
            for (int i = 0; i < 3; ++i) maps[at * 9 + i] = cand_k[3 * e0 + i], maps[at * 9 + 3 + i] = cand_k[3 * e1 + i], maps[at * 9 + 6 + i] = cand_k[3 * e2 + i];
        }
        nmaps += total;
    }
    __syncthreads();   // the map list is complete; the candidate lists are dead
    if (nmaps > SM_MAX_MAPS || nmaps == 0) {
        sm_fail(a, p, tid, nmaps == 0 ? SM_NO_LATTICE : SM_MAP_CAP_HIT, nmaps > SM_MAX_MAPS ? SM_MAX_MAPS : 0);
        return;
    }
    if (a.maps)
        for (int i = tid; i < nmaps * 9; i += SM_THREADS) a.maps[(size_t)p * SM_MAX_MAPS * 9 + i] = maps[i];
    // ---- the items
    const int* spec_off = a.a.spec_off + (size_t)q * (SM_MAX_SPECIES + 1);
    const int rarest = a.b.info[(size_t)c * 4 + 2];
    SmPair P{f1, f2, L1, L2, maps, spec_off, n, a.a.info[(size_t)q * 4 + 1], spec_off[rarest], spec_off[rarest + 1] - spec_off[rarest]};
    unsigned char* wb = sm_lds + Lds::waves + (size_t)wave * Lds::wave_bytes;
    SmWave W{reinterpret_cast<double*>(wb + Lds::tile), reinterpret_cast<double*>(wb + Lds::f2p), reinterpret_cast<double*>(wb + Lds::u),
             reinterpret_cast<double*>(wb + Lds::d2), reinterpret_cast<int*>(wb + Lds::col)};
    const int items = nmaps * P.ntrans;
    double best = sm_inf(), best_m = sm_inf();
    int best_i = SM_NO_COL;
    for (int item = wave; item < items; item += SM_WAVES) {   // (uniform per wave)
        double rms, md;
        sm_wave_item(P, W, item, lane, &rms, &md);
        if (sm_better(rms, item, best, best_i)) best = rms, best_m = md, best_i = item;
    }
    if (lane == 0) s_best_v[wave] = best, s_best_m[wave] = best_m, s_best_i[wave] = best_i;
    __syncthreads();
    best = s_best_v[0], best_m = s_best_m[0], best_i = s_best_i[0];
#pragma unroll
    for (int w = 1; w < SM_WAVES; ++w)
        if (sm_better(s_best_v[w], s_best_i[w], best, best_i)) best = s_best_v[w], best_m = s_best_m[w], best_i = s_best_i[w];
    const bool found = best_i != SM_NO_COL;   // (items >= 1, so only a pair whose every rms is not a number has none)
    if (tid == 0) {
        a.rms[p] = found ? best : sm_inf(), a.max_dist[p] = found ? best_m : sm_inf();
        a.best_trans[p] = found ? best_i % P.ntrans : -1;
        a.n_maps[p] = nmaps, a.n_items[p] = items, a.status[p] = SM_OK;
    }
    if (tid < 9) a.best_map[(size_t)p * 9 + tid] = found ? maps[(best_i / P.ntrans) * 9 + tid] : 0;
    if (a.perm && wave == 0) {
        double rms, md;
        const bool ok = found && sm_wave_item(P, W, best_i, lane, &rms, &md);
        sm_wave_sync();
        int* by_atom = reinterpret_cast<int*>(W.d2);   // the query's atoms in the caller's order
        if (ok && lane < n) by_atom[a.a.perm[n0a + lane]] = a.b.perm[n0b + W.col[lane]];
        sm_wave_sync();
        a.perm[(size_t)p * SM_MAX_ATOMS + lane] = (ok && lane < n) ? by_atom[lane] : -1;
    }
}

static int sm_prepared_check(const char* what, const mi_sm_prepared& s) {
    MI_CHECK(s.B >= 0 && s.N >= 0, MI_EINVAL, "%s: negative count (B %d, N %d)", what, s.B, s.N);
    if (s.B == 0) return MI_OK;
    MI_CHECK(s.offsets && s.lat && s.inv && s.frac && s.types && s.perm && s.spec_Z && s.spec_off && s.info, MI_EINVAL, "%s: null pointer in a prepared set", what);
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_sm_prepare(const int* types, const float* frac, const float* lat, const mi_sm_prepared* out, void* stream) {
    MI_CHECK(out, MI_EINVAL, "mi_sm_prepare: null prepared set");
    MI_TRY(sm_prepared_check("mi_sm_prepare", *out));
    if (out->B == 0) return MI_OK;
    MI_CHECK(lat && (out->N == 0 || (types && frac)), MI_EINVAL, "mi_sm_prepare: null input pointer");
    SmPrepArgs A{types, frac, lat, *out};
    hipLaunchKernelGGL(sm_prepare_kernel, dim3(out->B), dim3(64), 0, (hipStream_t)stream, A);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int mi_sm_match(const mi_sm_match_args* args, void* stream) {
    MI_CHECK(args, MI_EINVAL, "mi_sm_match: null argument block");
    const mi_sm_match_args& a = *args;
    MI_CHECK(a.P >= 0, MI_EINVAL, "mi_sm_match: P = %d", a.P);
    MI_CHECK(a.ltol >= 0.0 && a.ltol < 1.0, MI_EINVAL, "mi_sm_match: ltol = %g outside [0, 1)", a.ltol);
    MI_CHECK(a.cos_tol > 0.0 && a.cos_tol <= 1.0, MI_EINVAL, "mi_sm_match: cos_tol = %g outside (0, 1]", a.cos_tol);
    MI_TRY(sm_prepared_check("mi_sm_match", a.a));
    MI_TRY(sm_prepared_check("mi_sm_match", a.b));
    if (a.P == 0) return MI_OK;
    MI_CHECK(a.pair_q && a.pair_c && a.rms && a.max_dist && a.best_map && a.best_trans && a.n_maps && a.n_items && a.status, MI_EINVAL,
             "mi_sm_match: null pointer");
    MI_CHECK(a.a.B > 0 && a.b.B > 0, MI_EINVAL, "mi_sm_match: pairs into an empty set");
    static std::once_flag once;
    static hipError_t attr_err = hipSuccess;
    std::call_once(once, [] {
        attr_err = hipFuncSetAttribute((const void*)sm_match_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SmLds<64>::bytes);
        if (attr_err == hipSuccess)
            attr_err = hipFuncSetAttribute((const void*)sm_match_kernel<32>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SmLds<32>::bytes);
    });
    MI_HIP(attr_err);
    hipLaunchKernelGGL(sm_match_kernel<32>, dim3(a.P), dim3(SM_THREADS), SmLds<32>::bytes, (hipStream_t)stream, a);
    MI_KERNEL_CHECK();
    hipLaunchKernelGGL(sm_match_kernel<64>, dim3(a.P), dim3(SM_THREADS), SmLds<64>::bytes, (hipStream_t)stream, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // extern "C"
