// Energy above the convex hull (include/matinvent_hip_hull.h).  Launches of this unit, no atomics, no scratch, no matrix pipe:
//   hull_stage_kernel   one 256-thread workgroup per group: the group's candidates as a dense structure-of-arrays block (d columns of
//                       fractions in the group's element order, then the energies, and the bank rows) in the workspace, behind the guard;
//                       the query positions' group map and the group's flag;
//   hull_solve_kernel   one 256-thread workgroup per query position: the block in LDS when it fits HULL_LDS_DOUBLES, else read from the
//                       workspace; the terminals and every pricing step as a strided argmin of (value, position) through one fixed tree
//                       (xor butterfly inside a wave, then the four waves in order); one lane owns the d x d state in LDS.
// csrc/hull_simplex.h holds every formula, host and device.

#include "../../include/matinvent_hip_hull.h"
#include "common.h"
#include "hull_simplex.h"

namespace mi {

static_assert(HULL_MAX_ELEMS == MI_HULL_MAX_ELEMS && HULL_MAX_ITERS == MI_HULL_MAX_ITERS && HULL_LDS_DOUBLES == MI_HULL_LDS_DOUBLES, "sizes");
static_assert(HULL_OK == MI_HULL_OK && HULL_NO_TERMINAL == MI_HULL_NO_TERMINAL && HULL_UNBOUNDED == MI_HULL_UNBOUNDED &&
                  HULL_ITER_CAP == MI_HULL_ITER_CAP && HULL_BAD_QUERY == MI_HULL_BAD_QUERY && HULL_FLAG_SKIPPED == MI_HULL_FLAG_SKIPPED,
              "status codes");
static_assert(HULL_EPS == MI_HULL_EPS, "epsilons");

struct HullArgs {
    mi_hull_args a;
    double* ws_x;    // [nnz_c][HULL_COLS]: group g's block starts at element HULL_COLS * grp_c_off[g]
    int* ws_row;     // [nnz_c]
    int* ws_qgrp;    // [nnz_q]; -1: the position belongs to no admissible group
    int* ws_gflag;   // [G]
};

__global__ __launch_bounds__(HULL_THREADS) void hull_stage_kernel(HullArgs A) {
    const mi_hull_args& a = A.a;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int d = a.grp_nelem[g];
    const int* gZ = a.grp_Z + (size_t)g * HULL_MAX_ELEMS;
    const int q0 = a.grp_q_off[g], q1 = a.grp_q_off[g + 1], c0 = a.grp_c_off[g], c1 = a.grp_c_off[g + 1];
    if (!(hull_group_ok(gZ, d) && q0 >= 0 && q0 <= q1 && q1 <= a.nnz_q && c0 >= 0 && c0 <= c1 && c1 <= a.nnz_c)) return;   // (uniform)
    const HullBank bank{a.bank_nelem, a.bank_Z, a.bank_frac, a.bank_energy, a.M};
    const int nc = c1 - c0;
    int skipped = 0;
    for (int i = tid; i < nc; i += HULL_THREADS)
        skipped |= hull_stage_candidate(bank, gZ, d, a.c_idx[c0 + i], A.ws_x + (size_t)HULL_COLS * c0, A.ws_row + c0, nc, i);
    for (int p = q0 + tid; p < q1; p += HULL_THREADS) A.ws_qgrp[p] = g;
    skipped = __syncthreads_or(skipped);
    if (tid == 0) A.ws_gflag[g] = skipped ? HULL_FLAG_SKIPPED : 0;
}

// The block's argmin of (v, p) under hull_better, known to every thread on return.
__device__ __forceinline__ void hull_block_argmin(double& v, int& p, double* red_v, int* red_p, int tid) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(v, m, 64);
        const int op = __shfl_xor(p, m, 64);
        if (hull_better(ov, op, v, p)) v = ov, p = op;
    }
    if ((tid & 63) == 0) red_v[tid >> 6] = v, red_p[tid >> 6] = p;
    __syncthreads();
    v = red_v[0], p = red_p[0];
#pragma unroll
    for (int w = 1; w < HULL_THREADS / 64; ++w)
        if (hull_better(red_v[w], red_p[w], v, p)) v = red_v[w], p = red_p[w];
    __syncthreads();
}

__global__ __launch_bounds__(HULL_THREADS) void hull_solve_kernel(HullArgs A) {
    extern __shared__ __attribute__((aligned(16))) double hull_lds[];
    __shared__ HullState s;
    __shared__ double red_v[HULL_THREADS / 64];
    __shared__ int red_p[HULL_THREADS / 64];
    const mi_hull_args& a = A.a;
    const int pos = blockIdx.x, tid = threadIdx.x;
    const int g = A.ws_qgrp[pos];
    if (g < 0 || g >= a.G) return;   // (uniform) no admissible group owns this position
    const int q = a.q_idx[pos];
    if (q < 0 || q >= a.Q) return;   // (uniform)
    const int d = a.grp_nelem[g], c0 = a.grp_c_off[g], nc = a.grp_c_off[g + 1] - c0;
    const double* gx = A.ws_x + (size_t)HULL_COLS * c0;
    const int* rows = A.ws_row + c0;
    const int64_t cells = (int64_t)(d + 1) * nc;
    const bool in_lds = !a.no_lds && cells <= HULL_LDS_DOUBLES;
    if (in_lds) {
        for (int i = tid; i < (int)cells; i += HULL_THREADS) hull_lds[i] = gx[i];
    }
    if (tid < HULL_MAX_ELEMS) s.c[tid] = tid < d ? a.query_c[(size_t)q * HULL_MAX_ELEMS + tid] : 0.0;
    __syncthreads();
    const HullBlock blk{in_lds ? hull_lds : gx, rows, nc, d};
    for (int k = 0; k < d; ++k) {   // the terminals
        double v;
        int p;
        hull_terminal_thread(blk, k, tid, HULL_THREADS, v, p);
        hull_block_argmin(v, p, red_v, red_p, tid);
        if (tid == 0) s.basis[k] = p, s.EB[k] = v;
    }
    if (tid == 0) hull_start(s, d);
    __syncthreads();
    while (!s.done) {   // (uniform: s.done changes between the two barriers at the loop's end only)
        double y[HULL_MAX_ELEMS];
        int basis[HULL_MAX_ELEMS];
#pragma unroll
        for (int k = 0; k < HULL_MAX_ELEMS; ++k) {
            y[k] = k < d ? s.y[k] : 0.0;
            basis[k] = k < d ? s.basis[k] : -1;
        }
        double rmin;
        int j;
        hull_price_thread(blk, y, basis, tid, HULL_THREADS, rmin, j);
        hull_block_argmin(rmin, j, red_v, red_p, tid);
        if (tid == 0) {
            double Ej = 0.0;
            if (j != HULL_NO_POS) {
                for (int k = 0; k < d; ++k) s.xj[k] = hull_block_frac(blk, j, k);
                Ej = hull_block_energy(blk, j);
            }
            hull_decide(s, rmin, j, Ej);
        }
        __syncthreads();
    }
    const bool solved = s.status != HULL_NO_TERMINAL && s.status != HULL_BAD_QUERY;
    if (tid < HULL_MAX_ELEMS) {
        const bool live = solved && tid < d;
        a.chempot[(size_t)q * HULL_MAX_ELEMS + tid] = solved ? (tid < d ? s.y[tid] : 0.0) : hull_nan();
        a.decomp_frac[(size_t)q * HULL_MAX_ELEMS + tid] = live ? s.lam[tid] : 0.0;
        a.decomp_idx[(size_t)q * HULL_MAX_ELEMS + tid] = live ? rows[s.basis[tid]] : -1;
    }
    if (tid == 0) {
        const double e_hull = solved ? hull_value(s) : hull_nan();
        a.e_hull[q] = e_hull;
        a.e_above[q] = a.query_e[q] - e_hull;
        a.iters[q] = s.iters;
        a.status[q] = s.status;
        a.flags[q] = A.ws_gflag[g];
    }
}

static int64_t hull_align16(int64_t n) { return (n + 15) / 16 * 16; }

static int hull_launch(const mi_hull_args* args, hipStream_t stream) {
    MI_CHECK(args, MI_EINVAL, "hull: null argument block");
    const mi_hull_args& a = *args;
    MI_CHECK(a.M >= 0 && a.G >= 0 && a.Q >= 0 && a.nnz_q >= 0 && a.nnz_c >= 0, MI_EINVAL, "hull: negative count (M %d, G %d, Q %d, nnz_q %d, nnz_c %d)", a.M,
             a.G, a.Q, a.nnz_q, a.nnz_c);
    MI_CHECK(a.max_elems >= 1 && a.max_elems <= MI_HULL_MAX_ELEMS, MI_EINVAL, "hull: max_elems = %d outside 1..%d", a.max_elems, MI_HULL_MAX_ELEMS);
    MI_CHECK(a.e_hull && a.e_above && a.chempot && a.decomp_frac && a.decomp_idx && a.iters && a.status && a.flags, MI_EINVAL, "hull: null output pointer");
    MI_CHECK(a.bank_nelem && a.bank_Z && a.bank_frac && a.bank_energy && a.grp_nelem && a.grp_Z && a.grp_q_off && a.q_idx && a.grp_c_off && a.c_idx &&
                 a.query_c && a.query_e && a.workspace,
             MI_EINVAL, "hull: null input pointer");
    MI_CHECK(((uintptr_t)a.workspace & 15) == 0, MI_EINVAL, "hull: the workspace must be 16-byte aligned");
    if (a.G == 0 || a.Q == 0 || a.nnz_q == 0) return MI_OK;
    HullArgs A;
    A.a = a;
    char* w = (char*)a.workspace;
    A.ws_x = (double*)w;
    w += hull_align16((int64_t)a.nnz_c * HULL_COLS * (int64_t)sizeof(double));
    A.ws_row = (int*)w;
    w += hull_align16((int64_t)a.nnz_c * (int64_t)sizeof(int));
    A.ws_qgrp = (int*)w;
    w += hull_align16((int64_t)a.nnz_q * (int64_t)sizeof(int));
    A.ws_gflag = (int*)w;
    MI_HIP(hipMemsetAsync(A.ws_qgrp, 0xFF, (size_t)a.nnz_q * sizeof(int), stream));   // -1: a rejected group's positions stay unowned
    hipLaunchKernelGGL(hull_stage_kernel, dim3(a.G), dim3(HULL_THREADS), 0, stream, A);
    MI_KERNEL_CHECK();
    hipLaunchKernelGGL(hull_solve_kernel, dim3(a.nnz_q), dim3(HULL_THREADS), a.no_lds ? 0 : (size_t)HULL_LDS_DOUBLES * sizeof(double), stream, A);
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int64_t mi_hull_workspace(int G, int nnz_q, int nnz_c) {
    MI_CHECK(G >= 0 && nnz_q >= 0 && nnz_c >= 0, MI_EINVAL, "hull workspace: negative count (G %d, nnz_q %d, nnz_c %d)", G, nnz_q, nnz_c);
    return hull_align16((int64_t)nnz_c * HULL_COLS * (int64_t)sizeof(double)) + hull_align16((int64_t)nnz_c * (int64_t)sizeof(int)) +
           hull_align16((int64_t)nnz_q * (int64_t)sizeof(int)) + hull_align16((int64_t)G * (int64_t)sizeof(int)) + 16;
}

int mi_hull_above(const mi_hull_args* args, void* stream) { return hull_launch(args, (hipStream_t)stream); }

}  // extern "C"
