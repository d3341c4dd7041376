// The symmetry finder (include/matinvent_hip_sym.h).  Launches of this unit, no atomics, no scratch, no matrix pipe:
//   sym_find_kernel      one 256-thread workgroup per crystal: the self-maps of the reduced cell by the matcher's ordered compaction
//                        (ballot, wave counts in LDS) of the box points and of the candidate triples into LDS; then rounds of four
//                        (map, translation) items, one per wave, a lane per atom: the mapped coordinates in the wave's LDS, the nearest
//                        atom of the lane's species block, the bijection through one LDS slot per target; after a round's barrier every
//                        thread folds the four flags in item order (the counts, the distinct rotation parts and their classes) and the
//                        wave of an accepted item writes its operation;
//   sym_prim_kernel      one wave per crystal: the first basis triple of the translation lattice, a lane per third candidate; the orbit
//                        representatives, a lane per atom; the kept atoms, in the caller's order, into the workspace;
//   sym_scan_kernel      one workgroup: prim_offsets, the running sum of the kept counts;
//   sym_gather_kernel    one wave per crystal: workspace -> compacted outputs.
// csrc/sym_ops.h, sm_lattice.h and sm_assign.h hold every formula, host and device.

#include "../../include/matinvent_hip_sym.h"
#include "common.h"
#include "sym_ops.h"

namespace mi {

static_assert(SYM_MAX_OPS == MI_SYM_MAX_OPS && SYM_MAX_TRANS == MI_SYM_MAX_TRANS && SYM_INFO == MI_SYM_INFO && SYM_CLASSES == MI_SYM_CLASSES, "sizes");
static_assert(SYM_MAX_TRANS == SM_MAX_ATOMS, "a pure translation per atom of the rarest species at most");
static_assert(SYM_OK == MI_SYM_OK && SYM_NOT_PREPARED == MI_SYM_NOT_PREPARED && SYM_BOX_CAP == MI_SYM_BOX_CAP && SYM_MAP_CAP == MI_SYM_MAP_CAP &&
                  SYM_NO_LATTICE == MI_SYM_NO_LATTICE && SYM_AMBIGUOUS == MI_SYM_AMBIGUOUS && SYM_OPS_CAP == MI_SYM_OPS_CAP &&
                  SYM_NOT_A_GROUP == MI_SYM_NOT_A_GROUP && SYM_PRIM_FAIL == MI_SYM_PRIM_FAIL && SYM_BAD_TOL == MI_SYM_BAD_TOL,
              "status bits");

constexpr int SYM_WAVES = SM_THREADS / 64;

struct SymFindArgs {
    mi_sm_prepared s;
    const double* tol;
    double cos_tol;
    mi_sym_out o;
};

__device__ __forceinline__ int sym_lanes_below(uint64_t mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

// LDS written by other lanes of this wave is read next
__device__ __forceinline__ void sym_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// a crystal without operations: the status, zeroed counts and a zeroed histogram
__device__ __forceinline__ void sym_fail(const mi_sym_out& o, int b, int tid, int status) {
    if (tid < SYM_INFO) o.info[(size_t)b * SYM_INFO + tid] = tid == SYM_INFO - 1 ? status : 0;
    if (tid < SYM_CLASSES) o.rot_hist[(size_t)b * SYM_CLASSES + tid] = 0;
}

struct SymWave {
    double* fp;   // [64][3] the mapped coordinates
    double* u;    // [64][3] the displacements of a pure translation
    int* hit;     // [64] the lane that claimed a target
};

__global__ __launch_bounds__(SM_THREADS) void sym_find_kernel(SymFindArgs A) {
    __shared__ int s_maps[SM_MAX_MAPS * 9];
    __shared__ double s_cell[9];
    __shared__ double s_f[SM_MAX_ATOMS * 3];
    __shared__ int s_blk0[SM_MAX_ATOMS], s_blkn[SM_MAX_ATOMS];
    __shared__ double s_cand_v[3 * SM_MAX_CAND * 3], s_cand_len[3 * SM_MAX_CAND];
    __shared__ int s_cand_k[3 * SM_MAX_CAND * 3];
    __shared__ double s_fp[SYM_WAVES][SM_MAX_ATOMS * 3], s_u[SYM_WAVES][SM_MAX_ATOMS * 3];
    __shared__ int s_hit[SYM_WAVES][SM_MAX_ATOMS];
    __shared__ int s_count[2][3][SYM_WAVES];
    __shared__ int s_acc[2][SYM_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int* pinfo = A.s.info + (size_t)b * 4;
    if (pinfo[3] != SM_PREP_OK) {   // (uniform) nothing is read through this crystal's offsets
        sym_fail(A.o, b, tid, SYM_NOT_PREPARED);
        return;
    }
    const double tol = A.tol[b];
    if (!sym_tol_ok(tol)) {
        sym_fail(A.o, b, tid, SYM_BAD_TOL);
        return;
    }
    const int n = pinfo[0], nspec = pinfo[1], rarest = pinfo[2], n0 = A.s.offsets[b];
    const int* spec_off = A.s.spec_off + (size_t)b * (SM_MAX_SPECIES + 1);
    if (tid < 9) s_cell[tid] = A.s.lat[(size_t)b * 9 + tid];
    for (int i = tid; i < 3 * n; i += SM_THREADS) s_f[i] = A.s.frac[(size_t)n0 * 3 + i];
    if (tid < n) {
        int s = 0;
        for (int e = 1; e < nspec; ++e) s += spec_off[e] <= tid ? 1 : 0;
        s_blk0[tid] = spec_off[s], s_blkn[tid] = spec_off[s + 1] - spec_off[s];
    }
    __syncthreads();
    const double* L = s_cell;
    // ---- the candidate vectors of the three axes, in lexicographic order of k (the matcher's enumeration on (b, b))
    SmTarget tg;
    sm_target(L, &tg);
    int bound[3];
    const int pts = sym_box(tg, A.s.inv + (size_t)b * 9, tol, bound);
    if (pts < 0) {
        sym_fail(A.o, b, tid, SYM_BOX_CAP);
        return;
    }
    int ncand[3] = {0, 0, 0};
    int round = 0;
    for (int base = 0; base < pts; base += SM_THREADS, ++round) {
        const int pt = base + tid;
        int k[3] = {0, 0, 0};
        double v[3] = {0.0, 0.0, 0.0}, len = 0.0;
        if (pt < pts) sm_box_point(pt, bound, L, k, v, &len);
        uint64_t mask[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            mask[ax] = __ballot(pt < pts && sym_length_ok(len, tg.len[ax], tol));
            if (lane == 0) s_count[round & 1][ax][wave] = __popcll(mask[ax]);
        }
        __syncthreads();
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            int before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < SYM_WAVES; ++w) {
                const int cw = s_count[round & 1][ax][w];
                before += w < wave ? cw : 0, total += cw;
            }
            const int at = ncand[ax] + before + sym_lanes_below(mask[ax], lane);
            if (((mask[ax] >> lane) & 1ull) && at < SM_MAX_CAND) {
                const int e = ax * SM_MAX_CAND + at;
                s_cand_v[3 * e] = v[0], s_cand_v[3 * e + 1] = v[1], s_cand_v[3 * e + 2] = v[2], s_cand_len[e] = len;
                s_cand_k[3 * e] = k[0], s_cand_k[3 * e + 1] = k[1], s_cand_k[3 * e + 2] = k[2];
            }
            ncand[ax] += total;
        }
    }
    __syncthreads();
    if (ncand[0] > SM_MAX_CAND || ncand[1] > SM_MAX_CAND || ncand[2] > SM_MAX_CAND) {
        sym_fail(A.o, b, tid, SYM_BOX_CAP);
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
            ok = sm_triple_ok(tg, s_cand_v + 3 * e0, s_cand_len[e0], s_cand_k + 3 * e0, s_cand_v + 3 * e1, s_cand_len[e1], s_cand_k + 3 * e1, s_cand_v + 3 * e2,
                              s_cand_len[e2], s_cand_k + 3 * e2, A.cos_tol);
        }
        const uint64_t mask = __ballot(ok);
        if (lane == 0) s_count[round & 1][0][wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SYM_WAVES; ++w) {
            const int cw = s_count[round & 1][0][w];
            before += w < wave ? cw : 0, total += cw;
        }
        const int at = nmaps + before + sym_lanes_below(mask, lane);
        if (ok && at < SM_MAX_MAPS) {
#pragma unroll
            for (int i = 0; i < 3; ++i)
                s_maps[at * 9 + i] = s_cand_k[3 * e0 + i], s_maps[at * 9 + 3 + i] = s_cand_k[3 * e1 + i], s_maps[at * 9 + 6 + i] = s_cand_k[3 * e2 + i];
        }
        nmaps += total;
    }
    __syncthreads();
    if (nmaps > SM_MAX_MAPS || nmaps == 0) {
        sym_fail(A.o, b, tid, nmaps == 0 ? SYM_NO_LATTICE : SYM_MAP_CAP);
        return;
    }
    // ---- the items: rounds of four, one per wave, a lane per atom
    const int r0 = spec_off[rarest], ntrans = spec_off[rarest + 1] - spec_off[rarest];
    const int items = nmaps * ntrans;
    double G[9];
    sym_metric(L, G);
    const SymWave W{s_fp[wave], s_u[wave], s_hit[wave]};
    int n_ops = 0, n_trans = 0, pg_order = 0, last_map = -1, status = SYM_OK;
    int hist[SYM_CLASSES];
#pragma unroll
    for (int c = 0; c < SYM_CLASSES; ++c) hist[c] = 0;
    for (int base = 0; base < items; base += SYM_WAVES, ++round) {   // (uniform)
        const int item = base + wave;
        bool ok = false, amb = false, ident = false;
        double dev = 0.0, t[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0};
        int M[9];
        if (item < items) {   // (uniform per wave)
            const int m = item / ntrans, j = item - m * ntrans;
            int Mi[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) M[i] = s_maps[m * 9 + i];
            ident = sym_is_identity(M);
            sm_map_inverse(M, Mi);
            sym_wave_sync();   // the previous item's reads of W are done
            if (lane < n) {
                double f[3];
                sm_map_frac(s_f + 3 * lane, Mi, f);
                W.fp[3 * lane] = f[0], W.fp[3 * lane + 1] = f[1], W.fp[3 * lane + 2] = f[2];
            }
            sym_wave_sync();
#pragma unroll
            for (int c = 0; c < 3; ++c) t[c] = s_f[3 * (r0 + j) + c] - W.fp[3 * r0 + c];
            int tgt = 0;
            bool good = true;
            if (lane < n) {
                double d2;
                tgt = sym_nearest(G, s_f, s_blk0[lane], s_blkn[lane], W.fp + 3 * lane, t, u, &d2);
                dev = sqrt(d2);
                good = dev <= tol;
                W.hit[tgt] = lane;   // (of the lanes that share a target one stays)
            }
            const bool within = __all(good);
            sym_wave_sync();
            const bool bij = __all(lane >= n || W.hit[tgt] == lane);
            ok = within && bij, amb = within && !bij;
#pragma unroll
            for (int mk = 32; mk >= 1; mk >>= 1) {
                const double o = __shfl_xor(dev, mk, 64);
                dev = o > dev ? o : dev;
            }
        }
        if (lane == 0) s_acc[round & 1][wave] = (ok ? 1 : 0) | (amb ? 2 : 0);
        __syncthreads();
        int at_op = 0, at_tr = 0;
#pragma unroll
        for (int w = 0; w < SYM_WAVES; ++w) {   // the fold of the round in item order, every thread the same
            const int it = base + w;
            if (it >= items) continue;
            const int a = s_acc[round & 1][w];
            if (a & 2) status |= SYM_AMBIGUOUS;
            if (!(a & 1)) continue;
            const int m = it / ntrans;
            int Mw[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) Mw[i] = s_maps[m * 9 + i];
            if (m != last_map) {
                last_map = m, ++pg_order;
                const int cls = sym_class(Mw);
                if (cls < 0) status |= SYM_NOT_A_GROUP;
#pragma unroll
                for (int c = 0; c < SYM_CLASSES; ++c) hist[c] += c == cls ? 1 : 0;
            }
            if (w == wave) at_op = n_ops, at_tr = n_trans;
            ++n_ops;
            n_trans += sym_is_identity(Mw) ? 1 : 0;
        }
        if (ok) {   // (uniform per wave)
            if (at_op < SYM_MAX_OPS) {
                const size_t e = (size_t)b * SYM_MAX_OPS + at_op;
#pragma unroll
                for (int i = 0; i < 9; ++i)
                    if (lane == i) A.o.rot[e * 9 + i] = M[i];
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (lane == 9 + c) A.o.trans[e * 3 + c] = sm_wrap01(t[c]);
                if (lane == 12) A.o.dev[e] = dev;
            }
            if (ident) {   // a pure translation: refined by the mean displacement (at_tr < ntrans <= 64)
                if (lane < n) W.u[3 * lane] = u[0], W.u[3 * lane + 1] = u[1], W.u[3 * lane + 2] = u[2];
                sym_wave_sync();
                double mean[3];
                sm_mean(W.u, n, mean);
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (lane == c) A.o.ptrans[((size_t)b * SYM_MAX_TRANS + at_tr) * 3 + c] = sm_wrap01(t[c] - mean[c]);
            }
        }
    }
    if (n_ops > SYM_MAX_OPS) status |= SYM_OPS_CAP;
    if (n_ops != pg_order * n_trans) status |= SYM_NOT_A_GROUP;
    const int pg = sym_point_group(hist);
    if (pg == 0) status |= SYM_NOT_A_GROUP;   // the classes are those of no point group
    if (tid == 0) {
        int* oi = A.o.info + (size_t)b * SYM_INFO;
        oi[0] = n_ops, oi[1] = n_trans, oi[2] = nmaps, oi[3] = pg_order, oi[4] = pg, oi[5] = sym_crystal_system(pg), oi[6] = hist[4] > 0 ? 1 : 0, oi[7] = status;
    }
#pragma unroll
    for (int c = 0; c < SYM_CLASSES; ++c)
        if (tid == c) A.o.rot_hist[(size_t)b * SYM_CLASSES + c] = hist[c];
}

// ---- the primitive cell ----------------------------------------------------------------------------------------------------------------------
// the crystal unchanged into the workspace; any atom count
__device__ __forceinline__ void sym_prim_copy(const mi_sym_prim_args& a, int b, int lane, int n0, int n, int status) {
    for (int i = lane; i < n; i += 64) {
        a.ws_types[n0 + i] = a.types[n0 + i];
#pragma unroll
        for (int c = 0; c < 3; ++c) a.ws_frac[(size_t)(n0 + i) * 3 + c] = a.frac[(size_t)(n0 + i) * 3 + c];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i)
        if (lane == i) a.out_lat[(size_t)b * 9 + i] = a.lat[(size_t)b * 9 + i];
    if (lane == 0) a.prim_count[b] = n, a.prim_status[b] = status, a.prim_det[b] = 1.0;
}

__global__ __launch_bounds__(64) void sym_prim_kernel(mi_sym_prim_args a) {
    __shared__ double s_f[SM_MAX_ATOMS * 3], s_pt[SYM_MAX_TRANS * 3];
    __shared__ int s_keep[SM_MAX_ATOMS], s_src[SM_MAX_ATOMS];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n0 = a.set.offsets[b], n1 = a.set.offsets[b + 1];
    const int sym_status = a.sym_info[(size_t)b * SYM_INFO + SYM_INFO - 1], ntr = a.sym_info[(size_t)b * SYM_INFO + 1];
    if (!(n0 >= 0 && n0 <= n1 && n1 <= a.set.N)) {   // (uniform) nothing is read through these offsets
        sym_prim_copy(a, b, lane, 0, 0, sym_status);
        return;
    }
    const int n = n1 - n0;
    if ((sym_status & ~SYM_OPS_CAP) != SYM_OK || ntr <= 1 || ntr > SYM_MAX_TRANS || n > SM_MAX_ATOMS) {   // (past the cap the translations are all there)
        sym_prim_copy(a, b, lane, n0, n, sym_status);
        return;
    }
    for (int i = lane; i < 3 * n; i += 64) s_f[i] = a.set.frac[(size_t)n0 * 3 + i];
    for (int i = lane; i < 3 * ntr; i += 64) s_pt[i] = a.ptrans[(size_t)b * SYM_MAX_TRANS * 3 + i];
    __syncthreads();
    // ---- the first triple i < j < k of index n_trans, a lane per k
    const int m = ntr + 3;
    int bi = -1, bj = -1, bk = -1;
    for (int i = 0; i < m - 2 && bi < 0; ++i)
        for (int j = i + 1; j < m - 1 && bi < 0; ++j)
            for (int k0 = j + 1; k0 < m && bi < 0; k0 += 64) {
                const int k = k0 + lane;
                double P[9];
                const bool ok = k < m && sym_prim_det_ok(sym_prim_det(s_pt, ntr, i, j, k, P), ntr);
                const uint64_t mask = __ballot(ok);
                if (mask) bi = i, bj = j, bk = k0 + __builtin_ctzll(mask);
            }
    if (bi < 0) {
        sym_prim_copy(a, b, lane, n0, n, sym_status | SYM_PRIM_FAIL);
        return;
    }
    double P[9], Pinv[9];
    const double det = sym_prim_det(s_pt, ntr, bi, bj, bk, P);
    sm_inv3(P, det, Pinv);
    // ---- the orbit representatives, a lane per atom: kept when no translation carries the atom to a lower index
    const int* spec_off = a.set.spec_off + (size_t)b * (SM_MAX_SPECIES + 1);
    const int nspec = a.set.info[(size_t)b * 4 + 1];
    double G[9];
    {
        double Ls[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) Ls[i] = a.set.lat[(size_t)b * 9 + i];
        sym_metric(Ls, G);
    }
    bool keep = false;
    if (lane < n) {
        int s = 0;
        for (int e = 1; e < nspec; ++e) s += spec_off[e] <= lane ? 1 : 0;
        const int b0 = spec_off[s], nb = spec_off[s + 1] - b0;
        keep = true;
        for (int p = 1; p < ntr; ++p) {
            double u[3], d2;
            keep = keep && sym_nearest(G, s_f, b0, nb, s_f + 3 * lane, s_pt + 3 * p, u, &d2) > lane;
        }
        const int c = a.set.perm[n0 + lane];
        s_keep[c] = keep ? 1 : 0, s_src[c] = lane;
    }
    const int kept = __popcll(__ballot(keep));
    __syncthreads();
    if (kept * ntr != n) {
        sym_prim_copy(a, b, lane, n0, n, sym_status | SYM_PRIM_FAIL);
        return;
    }
    // ---- the kept atoms in the caller's order; the cell P x (T x the caller's cell)
    const bool mine = lane < n && s_keep[lane] != 0;
    const uint64_t kmask = __ballot(mine);
    if (mine) {
        const int at = n0 + __popcll(kmask & ((1ull << lane) - 1ull));
        float f32[3];
        sym_prim_frac(s_f + 3 * s_src[lane], Pinv, f32);
        a.ws_frac[(size_t)at * 3] = f32[0], a.ws_frac[(size_t)at * 3 + 1] = f32[1], a.ws_frac[(size_t)at * 3 + 2] = f32[2];
        a.ws_types[at] = a.types[n0 + lane];
    }
    int T[9];
    double L0[9], Lr[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) L0[i] = (double)a.lat[(size_t)b * 9 + i];
    sm_reduce(L0, T, Lr);   // (the prepare status is OK: the reduction ended)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double row[3];
        sym_prim_row(P, Lr, i, row);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (lane == 3 * i + c) a.out_lat[(size_t)b * 9 + 3 * i + c] = (float)row[c];
    }
    if (lane == 0) a.prim_count[b] = kept, a.prim_status[b] = sym_status, a.prim_det[b] = sm_abs(det);
}

// prim_offsets [B + 1]: the running sum of prim_count, chunks of 256 crystals with a carried total
__global__ __launch_bounds__(SM_THREADS) void sym_scan_kernel(const int* count, int* offsets, int B) {
    __shared__ int s_sum[2][SM_THREADS];
    const int tid = threadIdx.x;
    int carry = 0;
    if (tid == 0) offsets[0] = 0;
    for (int base = 0; base < B; base += SM_THREADS) {   // (uniform)
        int v = base + tid < B ? count[base + tid] : 0;
        int cur = 0;
        s_sum[cur][tid] = v;
        __syncthreads();
        for (int d = 1; d < SM_THREADS; d <<= 1) {
            const int o = s_sum[cur][tid] + (tid >= d ? s_sum[cur][tid - d] : 0);
            s_sum[cur ^ 1][tid] = o;
            cur ^= 1;
            __syncthreads();
        }
        if (base + tid < B) offsets[base + tid + 1] = carry + s_sum[cur][tid];
        carry += s_sum[cur][SM_THREADS - 1];
        __syncthreads();   // the next chunk rewrites s_sum
    }
}

__global__ __launch_bounds__(64) void sym_gather_kernel(mi_sym_prim_args a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int cnt = a.prim_count[b], dst = a.prim_offsets[b];
    if (cnt <= 0) return;
    const int n0 = a.set.offsets[b];   // (a crystal with atoms passed the offsets guard)
    for (int i = lane; i < cnt; i += 64) {
        if (dst + i >= a.set.N) break;   // (offsets that overlap: the compacted arrays hold N atoms)
        a.out_types[dst + i] = a.ws_types[n0 + i];
#pragma unroll
        for (int c = 0; c < 3; ++c) a.out_frac[(size_t)(dst + i) * 3 + c] = a.ws_frac[(size_t)(n0 + i) * 3 + c];
    }
}

static int sym_prepared_check(const char* what, const mi_sm_prepared& s) {
    MI_CHECK(s.B >= 0 && s.N >= 0, MI_EINVAL, "%s: negative count (B %d, N %d)", what, s.B, s.N);
    if (s.B == 0) return MI_OK;
    MI_CHECK(s.offsets && s.lat && s.inv && s.frac && s.types && s.perm && s.spec_Z && s.spec_off && s.info, MI_EINVAL, "%s: null pointer in a prepared set", what);
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_sym_find(const mi_sm_prepared* set, const double* tol, double cos_tol, const mi_sym_out* out, void* stream) {
    MI_CHECK(set && out, MI_EINVAL, "mi_sym_find: null argument block");
    MI_TRY(sym_prepared_check("mi_sym_find", *set));
    MI_CHECK(cos_tol > 0.0 && cos_tol <= 1.0, MI_EINVAL, "mi_sym_find: cos_tol = %g outside (0, 1]", cos_tol);
    if (set->B == 0) return MI_OK;
    MI_CHECK(tol && out->info && out->rot_hist && out->rot && out->trans && out->dev && out->ptrans, MI_EINVAL, "mi_sym_find: null pointer");
    SymFindArgs A{*set, tol, cos_tol, *out};
    hipLaunchKernelGGL(sym_find_kernel, dim3(set->B), dim3(SM_THREADS), 0, (hipStream_t)stream, A);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int mi_sym_primitive(const mi_sym_prim_args* args, void* stream) {
    MI_CHECK(args, MI_EINVAL, "mi_sym_primitive: null argument block");
    const mi_sym_prim_args& a = *args;
    MI_TRY(sym_prepared_check("mi_sym_primitive", a.set));
    if (a.set.B == 0) return MI_OK;
    MI_CHECK(a.lat && a.sym_info && a.ptrans && a.prim_count && a.prim_status && a.prim_det && a.prim_offsets && a.out_lat, MI_EINVAL,
             "mi_sym_primitive: null pointer");
    MI_CHECK(a.set.N == 0 || (a.types && a.frac && a.ws_types && a.ws_frac && a.out_types && a.out_frac), MI_EINVAL, "mi_sym_primitive: null atom array");
    hipLaunchKernelGGL(sym_prim_kernel, dim3(a.set.B), dim3(64), 0, (hipStream_t)stream, a);
    MI_KERNEL_CHECK();
    hipLaunchKernelGGL(sym_scan_kernel, dim3(1), dim3(SM_THREADS), 0, (hipStream_t)stream, (const int*)a.prim_count, a.prim_offsets, a.set.B);
    MI_KERNEL_CHECK();
    hipLaunchKernelGGL(sym_gather_kernel, dim3(a.set.B), dim3(64), 0, (hipStream_t)stream, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // extern "C"
