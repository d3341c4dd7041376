// The refined structure (include/matinvent_hip_sym_refine.h).  One launch, no atomics, no scratch, no matrix pipe:
//   sym_refine_kernel    one 256-thread workgroup per crystal, three phases between barriers.  A: the (operation, atom) items strided over
//                        the threads, each the nearest atom of the image in its species block, the site maps into LDS as bytes.  B: a
//                        thread per operation checks its map for a bijection and forms its refined translation from the pair costs of the
//                        known pairs; the last thread forms the mean metric and its Cholesky factor.  C: a thread per atom sums over the
//                        operations (the refined position, the orbit mask, the stabiliser count); fixed trees over LDS give the statistics.
//                        Nothing is written for a crystal before its checks are through: a failed crystal is copied as it came.
// The sums' orders are fixed by the definition, so the bits do not depend on the split into phases: the maps are kept, the residuals are
// formed again.  csrc/sym_refine.h holds every formula, host and device.

#include "../../include/matinvent_hip_sym_refine.h"
#include "common.h"
#include "sym_refine.h"

namespace mi {

static_assert(SYM_REFINE_FAIL == MI_SYM_REFINE_FAIL && REFINE_INFO == MI_SYM_REFINE_INFO && REFINE_STAT == MI_SYM_REFINE_STAT, "constants");
static_assert(SYM_MAX_OPS == MI_SYM_MAX_OPS && SYM_INFO == MI_SYM_INFO, "sizes");
static_assert(REFINE_ROW == SM_MAX_ATOMS && SM_MAX_ATOMS <= 64, "an atom is a byte of a row and a bit of a 64-bit mask");
static_assert(SYM_MAX_OPS < SM_THREADS && SM_MAX_ATOMS <= SM_THREADS, "a thread per operation and one more for the cell; a thread per atom");

// the info row and a zero statistics row
__device__ __forceinline__ void refine_rows(const mi_sym_refine_args& a, int b, int tid, int n_orbits, int n_ops, int status) {
    if (tid < REFINE_INFO) a.refine_info[(size_t)b * REFINE_INFO + tid] = tid == 0 ? n_orbits : (tid == 1 ? n_ops : (tid == REFINE_INFO - 1 ? status : 0));
    if (tid < REFINE_STAT) a.refine_stat[(size_t)b * REFINE_STAT + tid] = 0.0;
}

// the crystal as it came, bit for bit, every atom an orbit of its own
__device__ __forceinline__ void refine_copy(const mi_sym_refine_args& a, int b, int tid, int n0, int n, int n_ops, int status) {
    for (int i = tid; i < n; i += SM_THREADS) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.out_frac[(size_t)(n0 + i) * 3 + c] = a.frac[(size_t)(n0 + i) * 3 + c];
        a.orbit[n0 + i] = i, a.mult[n0 + i] = 1, a.site_order[n0 + i] = 1;
    }
    if (tid < 9) a.out_lat[(size_t)b * 9 + tid] = a.lat[(size_t)b * 9 + tid];
    refine_rows(a, b, tid, n, n_ops, status);
}

__global__ __launch_bounds__(SM_THREADS) void sym_refine_kernel(mi_sym_refine_args a) {
    __shared__ unsigned char s_sig[SYM_MAX_OPS * REFINE_ROW];
    __shared__ double s_f[SM_MAX_ATOMS * 3], s_t[SYM_MAX_OPS * 3], s_tbar[SYM_MAX_OPS * 3], s_G[9];
    __shared__ int s_rot[SYM_MAX_OPS * 9], s_perm[SM_MAX_ATOMS], s_blk0[SM_MAX_ATOMS], s_blkn[SM_MAX_ATOMS], s_T[9];
    __shared__ float s_lat[9];
    __shared__ double s_change;
    __shared__ double s_red[3][SM_THREADS];
    __shared__ int s_cnt[SM_THREADS], s_bad[SM_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int* sinfo = a.sym_info + (size_t)b * SYM_INFO;
    const int find_status = sinfo[SYM_INFO - 1], nops = sinfo[0];
    const int* pinfo = a.set.info + (size_t)b * 4;
    const int n = pinfo[0], nspec = pinfo[1];
    if (pinfo[3] != SM_PREP_OK || n < 1 || n > SM_MAX_ATOMS || nspec < 1 || nspec > SM_MAX_SPECIES) {   // (uniform) nothing is read through this crystal's offsets
        refine_rows(a, b, tid, 0, 0, find_status | SYM_NOT_PREPARED | SYM_REFINE_FAIL);
        return;
    }
    const int n0 = a.set.offsets[b];
    if (find_status != SYM_OK || nops < 1 || nops > SYM_MAX_OPS) {   // (uniform)
        refine_copy(a, b, tid, n0, n, nops, find_status | SYM_REFINE_FAIL);
        return;
    }
    if (nops == 1) {   // (uniform) the identity alone
        refine_copy(a, b, tid, n0, n, 1, find_status);
        return;
    }
    // ---- the crystal into LDS
    const int* spec_off = a.set.spec_off + (size_t)b * (SM_MAX_SPECIES + 1);
    bool bad = false;
    for (int i = tid; i < 3 * n; i += SM_THREADS) s_f[i] = a.set.frac[(size_t)n0 * 3 + i];
    for (int i = tid; i < 9 * nops; i += SM_THREADS) s_rot[i] = a.sym_rot[(size_t)b * SYM_MAX_OPS * 9 + i];
    for (int i = tid; i < 3 * nops; i += SM_THREADS) s_t[i] = a.sym_trans[(size_t)b * SYM_MAX_OPS * 3 + i];
    if (tid < n) {
        int b0, nb;
        refine_block(spec_off, nspec, tid, &b0, &nb);
        const int p = a.set.perm[n0 + tid];
        bad = b0 < 0 || nb < 1 || b0 + nb > n || tid < b0 || tid >= b0 + nb || p < 0 || p >= n;   // (a prepared set that is none)
        s_blk0[tid] = b0, s_blkn[tid] = nb, s_perm[tid] = bad ? 0 : p;
    }
    if (tid < 9) {
        double L[9], G[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) L[e] = a.set.lat[(size_t)b * 9 + e];
        sym_metric(L, G);
#pragma unroll
        for (int e = 0; e < 9; ++e)
            if (tid == e) s_G[e] = G[e];
    }
    s_bad[tid] = bad ? 1 : 0;
    __syncthreads();
    for (int s = SM_THREADS / 2; s >= 1; s >>= 1) {   // (uniform)
        if (tid < s) s_bad[tid] |= s_bad[tid + s];
        __syncthreads();
    }
    if (s_bad[0]) {   // (uniform)
        refine_copy(a, b, tid, n0, n, nops, find_status | SYM_REFINE_FAIL);
        return;
    }
    __syncthreads();   // s_bad is written again below
    double G[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) G[e] = s_G[e];
    // ---- A: the site maps; the largest squared residual of this thread's items
    double d2max = 0.0;
    for (int item = tid; item < nops * n; item += SM_THREADS) {
        const int k = item / n, i = item - k * n;
        double d2;
        const int at = refine_sigma(G, s_f, s_blk0[i], s_blkn[i], i, s_rot + 9 * k, s_t + 3 * k, &d2);
        s_sig[REFINE_ROW * k + i] = (unsigned char)at;   // (at is inside i's block: below n <= 64)
        d2max = refine_max(d2max, d2);
    }
    __syncthreads();
    // ---- B: a thread per operation: the bijection and the refined translation; the last thread: the cell
    bad = false;
    if (tid < nops) {
        bad = !refine_bijection(s_sig + REFINE_ROW * tid, n);
        double tb[3];
        refine_translation(G, s_f, n, s_sig + REFINE_ROW * tid, s_rot + 9 * tid, s_t + 3 * tid, tb);
        s_tbar[3 * tid] = tb[0], s_tbar[3 * tid + 1] = tb[1], s_tbar[3 * tid + 2] = tb[2];
    }
    if (tid == SM_THREADS - 1) {
        int T[9];
        float lat32[9], out[9];
        double Gbar[9], change;
#pragma unroll
        for (int e = 0; e < 9; ++e) lat32[e] = a.lat[(size_t)b * 9 + e];
        bad = !refine_cell(lat32, s_rot, nops, T, Gbar, &change, out);
#pragma unroll
        for (int e = 0; e < 9; ++e) s_T[e] = T[e], s_lat[e] = out[e];
        s_change = change;
    }
    __syncthreads();
    // ---- C: a thread per atom
    double xbar[3] = {0.0, 0.0, 0.0}, q = 0.0;
    int low = 0, mult = 0, stab = 0;
    if (tid < n) {
        refine_site(G, s_f, tid, s_sig, s_rot, s_tbar, nops, s_perm, xbar, &q, &low, &mult, &stab);
        bad = bad || mult * stab != nops;
    }
    s_bad[tid] = bad ? 1 : 0;
    s_cnt[tid] = tid < n && low == s_perm[tid] ? 1 : 0;   // the lowest atom of its orbit
    s_red[0][tid] = q, s_red[1][tid] = q, s_red[2][tid] = d2max;   // (q = 0 past the atoms)
    __syncthreads();
    for (int s = SM_THREADS / 2; s >= 1; s >>= 1) {   // (uniform) the fixed trees; the sum's 64 slots are its leaves, zeros above them
        if (tid < s) {
            s_bad[tid] |= s_bad[tid + s], s_cnt[tid] += s_cnt[tid + s];
            s_red[0][tid] = refine_max(s_red[0][tid], s_red[0][tid + s]);
            s_red[1][tid] = refine_tree_add(s_red[1][tid], s_red[1][tid + s]);
            s_red[2][tid] = refine_max(s_red[2][tid], s_red[2][tid + s]);
        }
        __syncthreads();
    }
    if (s_bad[0]) {   // (uniform)
        refine_copy(a, b, tid, n0, n, nops, find_status | SYM_REFINE_FAIL);
        return;
    }
    // ---- the outputs, in the caller's atom order
    if (tid < n) {
        int T[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) T[e] = s_T[e];
        float out[3];
        refine_frac(xbar, T, out);
        const int at = n0 + s_perm[tid];
#pragma unroll
        for (int c = 0; c < 3; ++c) a.out_frac[(size_t)at * 3 + c] = out[c];
        a.orbit[at] = low, a.mult[at] = mult, a.site_order[at] = stab;
    }
    if (tid < 9) a.out_lat[(size_t)b * 9 + tid] = s_lat[tid];
    for (int i = tid; i < 3 * nops; i += SM_THREADS) a.trans_ref[(size_t)b * SYM_MAX_OPS * 3 + i] = s_tbar[i];
    if (tid < REFINE_INFO) a.refine_info[(size_t)b * REFINE_INFO + tid] = tid == 0 ? s_cnt[0] : (tid == 1 ? nops : (tid == REFINE_INFO - 1 ? find_status : 0));
    if (tid < REFINE_STAT) {
        double row[REFINE_STAT];
        refine_stats(s_red[0][0], s_red[1][0], n, s_change, s_red[2][0], row);
#pragma unroll
        for (int e = 0; e < REFINE_STAT; ++e)
            if (tid == e) a.refine_stat[(size_t)b * REFINE_STAT + e] = row[e];
    }
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_sym_refine(const mi_sym_refine_args* args, void* stream) {
    MI_CHECK(args, MI_EINVAL, "mi_sym_refine: null argument block");
    const mi_sym_refine_args& a = *args;
    const mi_sm_prepared& s = a.set;
    MI_CHECK(s.B >= 0 && s.N >= 0, MI_EINVAL, "mi_sym_refine: negative count (B %d, N %d)", s.B, s.N);
    if (s.B == 0) return MI_OK;
    MI_CHECK(s.offsets && s.lat && s.inv && s.frac && s.types && s.perm && s.spec_Z && s.spec_off && s.info, MI_EINVAL,
             "mi_sym_refine: null pointer in a prepared set");
    MI_CHECK(a.lat && a.sym_info && a.sym_rot && a.sym_trans && a.out_lat && a.trans_ref && a.refine_info && a.refine_stat, MI_EINVAL, "mi_sym_refine: null pointer");
    MI_CHECK(s.N == 0 || (a.types && a.frac && a.out_frac && a.orbit && a.mult && a.site_order), MI_EINVAL, "mi_sym_refine: null atom array");
    hipLaunchKernelGGL(sym_refine_kernel, dim3(s.B), dim3(SM_THREADS), 0, (hipStream_t)stream, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // extern "C"
