// The substrate matcher (include/matinvent_hip_zsl.h).  Launches of this unit, no atomics, no scratch, no matrix pipe:
//   zsl_planes_kernel     one thread per (cell, plane): the reduced in-plane vectors, the area, the multiple count, the status;
//   zsl_tables_kernel     one 256-thread workgroup per plane: its superlattice entries (|a|, |b|, theta) for n = 1 .. mult, a thread per
//                         entry; the status gains REDUCE_CAP through one workgroup-wide OR;
//   zsl_search_kernel     one 256-thread workgroup per (film, film plane, substrate plane): n_f ascends in the outer loop, the film's
//                         entries of n_f staged in LDS, the threads stride over (film HNF x substrate HNF) of every admissible n_s, the
//                         substrate's entries read from its table; the exact minimum of the packed tie key, the int64 match count and the
//                         (strain, key) argmin go through one fixed tree (wave butterflies, then the four wave results in LDS);
//   zsl_reduce_kernel     one thread per (film, substrate plane): the film planes in ascending order;
//   zsl_mcia_kernel       one thread per (film, substrate): the substrate's planes in ascending order.
// csrc/zsl_match.h holds every formula, host and device.  The lowest match needs no knowledge of other items (an item never skips an n_f
// because another film plane found a smaller area): the result does not depend on launch order.

#include "../../include/matinvent_hip_zsl.h"
#include "common.h"
#include "zsl_match.h"

namespace mi {

static_assert(ZSL_MAX_MULT == MI_ZSL_MAX_MULT && ZSL_MAX_MILLER == MI_ZSL_MAX_MILLER && ZSL_TABLE == MI_ZSL_TABLE && ZSL_ROW_D == MI_ZSL_ROW_D &&
                  ZSL_ROW_I == MI_ZSL_ROW_I, "sizes");
static_assert(ZSL_OK == MI_ZSL_OK && ZSL_NO_MATCH == MI_ZSL_NO_MATCH && ZSL_MULT_CAP == MI_ZSL_MULT_CAP && ZSL_REDUCE_CAP == MI_ZSL_REDUCE_CAP &&
                  ZSL_BAD_CELL == MI_ZSL_BAD_CELL, "status codes");
static_assert(ZSL_MAX_HNF <= 255 && ZSL_MAX_MULT <= 63, "the packed tie key");

constexpr int ZSL_WAVES = ZSL_THREADS / 64;

__constant__ ZslCounts zsl_c = zsl_counts();

__global__ __launch_bounds__(ZSL_THREADS) void zsl_planes_kernel(mi_zsl_planes_args A, int T) {
    const int t = blockIdx.x * ZSL_THREADS + threadIdx.x;
    if (t >= T) return;
    int cell, p;
    if (A.cell_of) {
        cell = A.cell_of[t], p = t;
    } else {
        cell = t / A.P, p = t - cell * A.P;
    }
    double vec[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, area = 0.0;
    int mult = 0, status = ZSL_BAD_CELL;
    if (cell >= 0 && cell < A.C) {
        const int hkl[3] = {A.hkl[(size_t)p * 3], A.hkl[(size_t)p * 3 + 1], A.hkl[(size_t)p * 3 + 2]};
        float lat[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) lat[i] = A.lat[(size_t)cell * 9 + i];
        status = zsl_plane(lat, hkl, A.max_area, vec, &area, &mult);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) A.vec[(size_t)t * 6 + i] = vec[i];
    A.area[t] = area, A.mult[t] = mult, A.status[t] = status;
}

// mult and status as the kernels trust them: inside their ranges whatever the buffers hold
__device__ __forceinline__ int zsl_clamp_mult(int m) { return m < 0 ? 0 : m > ZSL_MAX_MULT ? ZSL_MAX_MULT : m; }
__device__ __forceinline__ int zsl_clamp_status(int s) { return s < ZSL_OK || s > ZSL_BAD_CELL ? ZSL_BAD_CELL : s; }

__global__ __launch_bounds__(ZSL_THREADS) void zsl_tables_kernel(const double* vec, const int* mult, int* status, double* table) {
    const int t = blockIdx.x, tid = threadIdx.x;
    const int st = zsl_clamp_status(status[t]);
    if (st == ZSL_BAD_CELL) return;   // (uniform) no entries; the status stays
    const int m = zsl_clamp_mult(mult[t]);
    const int* s_off = zsl_c.off;   // s_off[n]: the first entry of multiple n
    double v[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = vec[(size_t)t * 6 + i];
    const int entries = m >= 1 ? s_off[m + 1] : 0;
    bool cap = false;
    for (int e = tid; e < entries; e += ZSL_THREADS) {
        int n = 1;
        while (s_off[n + 1] <= e) ++n;   // (n <= m: e < s_off[m + 1])
        int i, j, w;
        zsl_hnf(n, e - s_off[n], &i, &j, &w);
        double out[3];
        cap = !zsl_super(v, i, j, w, out) || cap;
        double* dst = table + ((size_t)t * ZSL_TABLE + e) * 3;
        dst[0] = out[0], dst[1] = out[1], dst[2] = out[2];
    }
    const int any = __syncthreads_or(cap ? 1 : 0);
    if (tid == 0 && any) status[t] = zsl_max(st, ZSL_REDUCE_CAP);
}

// ---- the fixed tree: a butterfly inside each wave, then the four wave results in LDS, folded in wave order by every thread ----------------------
struct ZslTree {
    int* i;         // [ZSL_WAVES]
    double* d;      // [ZSL_WAVES]
    long long* n;   // [ZSL_WAVES]
};

__device__ __forceinline__ int zsl_block_min(int v, const ZslTree& T, int wave, int lane) {
#pragma unroll
    for (int mk = 32; mk >= 1; mk >>= 1) {
        const int o = __shfl_xor(v, mk, 64);
        v = o < v ? o : v;
    }
    __syncthreads();   // the tree's previous readers are done
    if (lane == 0) T.i[wave] = v;
    __syncthreads();
    int r = T.i[0];
#pragma unroll
    for (int w = 1; w < ZSL_WAVES; ++w) r = T.i[w] < r ? T.i[w] : r;
    return r;
}

__device__ __forceinline__ long long zsl_block_sum(long long v, const ZslTree& T, int wave, int lane) {
#pragma unroll
    for (int mk = 32; mk >= 1; mk >>= 1) v += __shfl_xor(v, mk, 64);
    __syncthreads();
    if (lane == 0) T.n[wave] = v;
    __syncthreads();
    long long r = T.n[0];
#pragma unroll
    for (int w = 1; w < ZSL_WAVES; ++w) r += T.n[w];
    return r;
}

__device__ __forceinline__ void zsl_block_argmin(double& v, int& k, const ZslTree& T, int wave, int lane) {
#pragma unroll
    for (int mk = 32; mk >= 1; mk >>= 1) {
        const double ov = __shfl_xor(v, mk, 64);
        const int ok = __shfl_xor(k, mk, 64);
        if (zsl_better(ov, ok, v, k)) v = ov, k = ok;
    }
    __syncthreads();
    if (lane == 0) T.d[wave] = v, T.i[wave] = k;
    __syncthreads();
    v = T.d[0], k = T.i[0];
#pragma unroll
    for (int w = 1; w < ZSL_WAVES; ++w)
        if (zsl_better(T.d[w], T.i[w], v, k)) v = T.d[w], k = T.i[w];
}

// an item without a match: thread 0 writes its rows
__device__ __forceinline__ void zsl_item_empty(const mi_zsl_search_args& A, size_t item, int flag) {
    double* d = A.item_d + item * ZSL_ROW_D;
    int* r = A.item_i + item * ZSL_ROW_I;
    d[0] = zsl_inf(), d[1] = zsl_nan(), d[2] = zsl_nan(), d[3] = zsl_nan(), d[4] = zsl_inf(), d[5] = zsl_inf(), d[6] = zsl_nan(), d[7] = zsl_nan(), d[8] = zsl_nan(),
    d[9] = 0.0;
#pragma unroll
    for (int i = 0; i < ZSL_ROW_I; ++i) r[i] = 0;
    r[0] = flag, r[1] = -1, r[10] = -1;
    A.item_n[item] = A.count ? 0 : -1;
}

__global__ __launch_bounds__(ZSL_THREADS) void zsl_search_kernel(mi_zsl_search_args A) {
    __shared__ double s_film[ZSL_MAX_HNF * 3];
    __shared__ int s_adm[ZSL_MAX_MULT + 1];
    __shared__ int s_ti[ZSL_WAVES];
    __shared__ double s_td[ZSL_WAVES];
    __shared__ long long s_tn[ZSL_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t item = blockIdx.x;
    const int sp = (int)(item % (size_t)A.Ps), fp = (int)((item / (size_t)A.Ps) % (size_t)A.Pf);
    const size_t fpl = item / (size_t)A.Ps;   // b * Pf + fp
    const int fst = zsl_clamp_status(A.f_status[fpl]), sst = zsl_clamp_status(A.s_status[sp]);
    if (fst == ZSL_BAD_CELL || sst == ZSL_BAD_CELL) {   // (uniform)
        if (tid == 0) zsl_item_empty(A, item, ZSL_BAD_CELL);
        return;
    }
    const int mf = zsl_clamp_mult(A.f_mult[fpl]), ms = zsl_clamp_mult(A.s_mult[sp]);
    const double Af = A.f_area[fpl], As = A.s_area[sp];
    double vec[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) vec[i] = A.f_vec[fpl * 6 + i];
    const double* table = A.s_table + (size_t)sp * ZSL_TABLE * 3;
    const int *s_sig = zsl_c.sig, *s_off = zsl_c.off;
    const ZslTree T{s_ti, s_td, s_tn};
    int lowest = ZSL_NO_KEY, best_key = ZSL_NO_KEY;
    double best_strain = zsl_inf();
    long long matches = 0;
    bool cap = false;
    for (int nf = 1; nf <= mf; ++nf) {   // (uniform)
        __syncthreads();   // the previous multiple's readers of s_film and s_adm are done
        const int sig_f = s_sig[nf];
        for (int h = tid; h < sig_f; h += ZSL_THREADS) {
            int i, j, w;
            zsl_hnf(nf, h, &i, &j, &w);
            double e[3];
            cap = !zsl_super(vec, i, j, w, e) || cap;
            s_film[3 * h] = e[0], s_film[3 * h + 1] = e[1], s_film[3 * h + 2] = e[2];
        }
        if (tid >= 1 && tid <= ms) s_adm[tid] = zsl_admissible(Af, As, nf, tid, A.max_area_ratio_tol) ? 1 : 0;
        __syncthreads();
        int key = ZSL_NO_KEY;
        for (int ns = 1; ns <= ms; ++ns) {   // (uniform)
            if (!s_adm[ns]) continue;
            const int sig_s = s_sig[ns], pairs = sig_f * sig_s;
            const double* sub = table + 3 * (size_t)s_off[ns];
            for (int t = tid; t < pairs; t += ZSL_THREADS) {
                const int h = t / sig_s, g = t - h * sig_s;
                double s[3];
                if (zsl_match(s_film + 3 * h, sub + 3 * g, A.max_length_tol, A.max_angle_tol, s)) {
                    const int k = zsl_key(nf, h, ns, g);
                    key = k < key ? k : key;
                    if (A.count) {
                        ++matches;
                        const double strain = zsl_strain(s);
                        if (zsl_better(strain, k, best_strain, best_key)) best_strain = strain, best_key = k;
                    }
                }
            }
        }
        if (lowest == ZSL_NO_KEY) {   // (uniform: every thread holds the tree's result)
            lowest = zsl_block_min(key, T, wave, lane);
            if (lowest != ZSL_NO_KEY && !A.count) break;
        }
    }
    const int any_cap = __syncthreads_or(cap ? 1 : 0);
    if (A.count) {
        matches = zsl_block_sum(matches, T, wave, lane);
        zsl_block_argmin(best_strain, best_key, T, wave, lane);
    }
    if (tid != 0) return;
    double* d = A.item_d + item * ZSL_ROW_D;
    int* r = A.item_i + item * ZSL_ROW_I;
    r[0] = zsl_max(zsl_max(fst, sst), any_cap ? ZSL_REDUCE_CAP : ZSL_OK);
    zsl_write_match(lowest, fp, vec, Af, table, s_off, A.max_length_tol, A.max_angle_tol, d, r + 1);
    if (A.count && best_key != ZSL_NO_KEY) {
        d[4] = best_strain;
        zsl_write_match(best_key, fp, vec, Af, table, s_off, A.max_length_tol, A.max_angle_tol, d + 5, r + 10);
    } else {
        d[4] = zsl_inf();
        zsl_write_match(ZSL_NO_KEY, fp, vec, Af, table, s_off, A.max_length_tol, A.max_angle_tol, d + 5, r + 10);
    }
    d[9] = 0.0, r[19] = 0;
    A.item_n[item] = A.count ? matches : -1;
}

// the status of a row: the largest flag, or OK / NO_MATCH when there is none
__device__ __forceinline__ int zsl_row_status(int flag, bool found) { return flag != ZSL_OK ? flag : found ? ZSL_OK : ZSL_NO_MATCH; }

__global__ __launch_bounds__(ZSL_THREADS) void zsl_reduce_kernel(mi_zsl_reduce_args A) {
    const size_t t = (size_t)blockIdx.x * ZSL_THREADS + threadIdx.x;
    if (t >= (size_t)A.B * A.Ps) return;
    const size_t b = t / (size_t)A.Ps;
    const int sp = (int)(t - b * (size_t)A.Ps);
    int flag = ZSL_OK, low = -1, ls = -1;
    double area = zsl_inf(), strain = zsl_inf();
    long long n = 0;
    for (int fp = 0; fp < A.Pf; ++fp) {
        const size_t item = (b * A.Pf + fp) * (size_t)A.Ps + sp;
        flag = zsl_max(flag, zsl_clamp_status(A.item_i[item * ZSL_ROW_I]));
        const double a = A.item_d[item * ZSL_ROW_D], s = A.item_d[item * ZSL_ROW_D + 4];
        if (a < area) area = a, low = fp;
        if (s < strain) strain = s, ls = fp;
        n += A.item_n[item];
    }
    double* d = A.res_d + t * ZSL_ROW_D;
    int* r = A.res_i + t * ZSL_ROW_I;
    const size_t il = (b * A.Pf + (low < 0 ? 0 : low)) * (size_t)A.Ps + sp, is = (b * A.Pf + (ls < 0 ? 0 : ls)) * (size_t)A.Ps + sp;
    // (without a match every item of the column holds the same empty half-row: item 0's is copied)
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = A.item_d[il * ZSL_ROW_D + i];
#pragma unroll
    for (int i = 4; i < ZSL_ROW_D; ++i) d[i] = A.item_d[is * ZSL_ROW_D + i];
#pragma unroll
    for (int i = 1; i < 10; ++i) r[i] = A.item_i[il * ZSL_ROW_I + i];
#pragma unroll
    for (int i = 10; i < ZSL_ROW_I; ++i) r[i] = A.item_i[is * ZSL_ROW_I + i];
    r[0] = zsl_row_status(flag, low >= 0);
    A.res_n[t] = A.count ? n : -1;
}

__global__ __launch_bounds__(ZSL_THREADS) void zsl_mcia_kernel(mi_zsl_reduce_args A) {
    const size_t t = (size_t)blockIdx.x * ZSL_THREADS + threadIdx.x;
    if (t >= (size_t)A.B * A.S) return;
    const size_t b = t / (size_t)A.S;
    const int s = (int)(t - b * (size_t)A.S);
    int p0 = A.sub_off[s], p1 = A.sub_off[s + 1];
    p0 = p0 < 0 ? 0 : p0, p1 = p1 > A.Ps ? A.Ps : p1;   // nothing is read outside the bank's planes
    int flag = ZSL_OK, plane = -1;
    double area = zsl_inf();
    for (int sp = p0; sp < p1; ++sp) {
        const int st = zsl_clamp_status(A.res_i[(b * A.Ps + sp) * ZSL_ROW_I]);
        flag = zsl_max(flag, st >= ZSL_MULT_CAP ? st : ZSL_OK);
        const double a = A.res_d[(b * A.Ps + sp) * ZSL_ROW_D];
        if (a < area) area = a, plane = sp;
    }
    A.mcia[t] = area, A.mcia_plane[t] = plane, A.mcia_status[t] = zsl_row_status(flag, plane >= 0);
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_zsl_planes(const mi_zsl_planes_args* args, void* stream) {
    MI_CHECK(args, MI_EINVAL, "mi_zsl_planes: null argument block");
    const mi_zsl_planes_args& a = *args;
    MI_CHECK(a.C >= 0 && a.P >= 0, MI_EINVAL, "mi_zsl_planes: negative count (C %d, P %d)", a.C, a.P);
    MI_CHECK(a.max_area > 0.0 && a.max_area - a.max_area == 0.0, MI_EINVAL, "mi_zsl_planes: max_area = %g is not positive and finite", a.max_area);
    const int64_t T = a.cell_of ? (int64_t)a.P : (int64_t)a.C * a.P;
    MI_CHECK(T <= 0x7fffffffLL, MI_EINVAL, "mi_zsl_planes: %lld planes", (long long)T);
    if (T == 0) return MI_OK;
    MI_CHECK(a.hkl && a.vec && a.area && a.mult && a.status && (a.lat || a.C == 0), MI_EINVAL, "mi_zsl_planes: null pointer");
    hipLaunchKernelGGL(zsl_planes_kernel, dim3(cdiv(T, ZSL_THREADS)), dim3(ZSL_THREADS), 0, (hipStream_t)stream, a, (int)T);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int64_t mi_zsl_workspace(int planes) {
    MI_CHECK(planes >= 0, MI_EINVAL, "mi_zsl_workspace: %d planes", planes);
    return (int64_t)planes * ZSL_TABLE * 3 * (int64_t)sizeof(double);
}

int mi_zsl_tables(const double* vec, const int* mult, int* status, int T, double* table, void* stream) {
    MI_CHECK(T >= 0, MI_EINVAL, "mi_zsl_tables: %d planes", T);
    if (T == 0) return MI_OK;
    MI_CHECK(vec && mult && status && table, MI_EINVAL, "mi_zsl_tables: null pointer");
    hipLaunchKernelGGL(zsl_tables_kernel, dim3(T), dim3(ZSL_THREADS), 0, (hipStream_t)stream, vec, mult, status, table);
    MI_KERNEL_CHECK();
    return MI_OK;
}

static int zsl_tol_ok(double v) { return v >= 0.0 && v - v == 0.0; }

int mi_zsl_search(const mi_zsl_search_args* args, void* stream) {
    MI_CHECK(args, MI_EINVAL, "mi_zsl_search: null argument block");
    const mi_zsl_search_args& a = *args;
    MI_CHECK(a.B >= 0 && a.Pf >= 0 && a.Ps >= 0, MI_EINVAL, "mi_zsl_search: negative count (B %d, Pf %d, Ps %d)", a.B, a.Pf, a.Ps);
    MI_CHECK(zsl_tol_ok(a.max_area_ratio_tol) && zsl_tol_ok(a.max_length_tol) && zsl_tol_ok(a.max_angle_tol), MI_EINVAL,
             "mi_zsl_search: a tolerance is negative or not finite (%g, %g, %g)", a.max_area_ratio_tol, a.max_length_tol, a.max_angle_tol);
    const double items = (double)a.B * (double)a.Pf * (double)a.Ps;
    MI_CHECK(items <= 2147483647.0, MI_ECAPACITY, "mi_zsl_search: %.0f items", items);
    if (items == 0.0) return MI_OK;
    MI_CHECK(a.f_vec && a.f_area && a.f_mult && a.f_status && a.s_area && a.s_mult && a.s_status && a.s_table && a.item_d && a.item_i && a.item_n, MI_EINVAL,
             "mi_zsl_search: null pointer");
    hipLaunchKernelGGL(zsl_search_kernel, dim3((unsigned)items), dim3(ZSL_THREADS), 0, (hipStream_t)stream, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int mi_zsl_reduce(const mi_zsl_reduce_args* args, void* stream) {
    MI_CHECK(args, MI_EINVAL, "mi_zsl_reduce: null argument block");
    const mi_zsl_reduce_args& a = *args;
    MI_CHECK(a.B >= 0 && a.Pf >= 1 && a.Ps >= 0 && a.S >= 0, MI_EINVAL, "mi_zsl_reduce: negative count or no film plane (B %d, Pf %d, Ps %d, S %d)", a.B, a.Pf, a.Ps, a.S);
    MI_CHECK((double)a.B * (double)a.Pf * (double)a.Ps <= 2147483647.0, MI_ECAPACITY, "mi_zsl_reduce: too many items");
    if (a.B == 0) return MI_OK;
    if (a.Ps > 0) {
        MI_CHECK(a.res_d && a.res_i && a.res_n && a.item_d && a.item_i && a.item_n, MI_EINVAL, "mi_zsl_reduce: null pointer");
        hipLaunchKernelGGL(zsl_reduce_kernel, dim3(cdiv((int64_t)a.B * a.Ps, ZSL_THREADS)), dim3(ZSL_THREADS), 0, (hipStream_t)stream, a);
        MI_KERNEL_CHECK();
    }
    if (a.S > 0) {
        MI_CHECK(a.sub_off && a.mcia && a.mcia_plane && a.mcia_status && (a.Ps == 0 || (a.res_d && a.res_i)), MI_EINVAL, "mi_zsl_reduce: null pointer");
        hipLaunchKernelGGL(zsl_mcia_kernel, dim3(cdiv((int64_t)a.B * a.S, ZSL_THREADS)), dim3(ZSL_THREADS), 0, (hipStream_t)stream, a);
        MI_KERNEL_CHECK();
    }
    return MI_OK;
}

}  // extern "C"
