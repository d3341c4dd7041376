// The conventional cell (include/matinvent_hip_sym_conv.h).  Launches of this unit, no atomics, no scratch, no matrix pipe:
//   sym_conv_basis_kernel    one wave per crystal: a lane per operation classifies the rotation parts the operation before did not have
//                            (order and axis of the proper part, into LDS); lane 0 folds them in operation order into the axis lists in
//                            LDS; then every lane runs the basis by crystal system, the searches of the box a lane per candidate with the
//                            minimum of (length, index) through one xor tree; the centring, the Bravais index, adj(M T) and the cell;
//   sym_conv_scan_kernel     one workgroup: conv_offsets, the running sum of the counts;
//   sym_conv_gather_kernel   one thread per output atom: its crystal by bisection of conv_offsets, copy j of atom i.
// csrc/sym_conv.h holds every formula, host and device.

#include "../../include/matinvent_hip_sym_conv.h"
#include "common.h"
#include "sym_conv.h"

namespace mi {

static_assert(SYM_CONV_FAIL == MI_SYM_CONV_FAIL && CONV_INFO == MI_SYM_CONV_INFO && CONV_MAX_MULT == MI_SYM_CONV_MAX_MULT, "constants");
static_assert(SYM_MAX_OPS == MI_SYM_MAX_OPS && SYM_INFO == MI_SYM_INFO, "sizes");

constexpr int CONV_POINTS = (2 * CONV_BOX + 1) * (2 * CONV_BOX + 1) * (2 * CONV_BOX + 1);

// the search of conv_basis over the lanes of one wave: every lane calls it, every lane gets the same point
struct ConvWaveSearch {
    const double* G;
    int lane;
    __host__ __device__ int operator()(const int* S, const int* excl, bool use_excl) const {
#if defined(__HIP_DEVICE_COMPILE__)
        double best = sm_inf();
        int bp = CONV_NO_POINT;
        for (int p = lane; p < CONV_POINTS; p += 64) {
            double l2;
            if (conv_cand(p, CONV_BOX, S, excl, use_excl, G, &l2) && sm_better(l2, p, best, bp)) best = l2, bp = p;
        }
#pragma unroll
        for (int mk = 32; mk >= 1; mk >>= 1) {
            const double o = __shfl_xor(best, mk, 64);
            const int op = __shfl_xor(bp, mk, 64);
            if (sm_better(o, op, best, bp)) best = o, bp = op;
        }
        return bp == CONV_NO_POINT ? -1 : bp;
#else
        (void)S, (void)excl, (void)use_excl;
        return -1;
#endif
    }
};

// a crystal without a conventional basis: bravais 0, M = I, one copy of every atom; with n = 0 and no cell for a crystal the prepare guard
// rejected
__device__ __forceinline__ void conv_fail(const mi_sym_conv_args& a, int b, int lane, int n, int system, int n_axes, int status, bool cell) {
    if (lane < CONV_INFO) {
        const int row[CONV_INFO] = {0, CONV_NONE, 1, system, n_axes, 1, 0, status};
        int v = 0;
#pragma unroll
        for (int i = 0; i < CONV_INFO; ++i) v = lane == i ? row[i] : v;
        a.conv_info[(size_t)b * CONV_INFO + lane] = v;
    }
    if (lane < 9) {
        a.conv_M[(size_t)b * 9 + lane] = lane % 4 == 0 ? 1 : 0, a.ws_adj[(size_t)b * 9 + lane] = lane % 4 == 0 ? 1 : 0;
        if (cell) a.out_lat[(size_t)b * 9 + lane] = a.lat[(size_t)b * 9 + lane];
    }
    if (lane < CONV_MAX_MULT * 3) a.conv_cvec[(size_t)b * CONV_MAX_MULT * 3 + lane] = 0;
    if (lane == 0) a.conv_count[b] = n;
}

__global__ __launch_bounds__(64) void sym_conv_basis_kernel(mi_sym_conv_args a) {
    __shared__ int s_order[SYM_MAX_OPS], s_axis[SYM_MAX_OPS * 3];
    __shared__ ConvAxes s_ax;
    __shared__ int s_cvec[64][CONV_MAX_MULT * 3];   // (a row per lane: every lane forms the same list)
    const int b = blockIdx.x, lane = threadIdx.x;
    const int* sinfo = a.sym_info + (size_t)b * SYM_INFO;
    const int find_status = sinfo[SYM_INFO - 1], system = sinfo[5], nops = sinfo[0];
    const int* pinfo = a.set.info + (size_t)b * 4;
    if (pinfo[3] != SM_PREP_OK) {   // (uniform) nothing is read through this crystal's offsets
        conv_fail(a, b, lane, 0, 0, 0, find_status | SYM_NOT_PREPARED | SYM_CONV_FAIL, false);
        return;
    }
    const int n = pinfo[0];
    if (find_status != SYM_OK || nops < 1 || nops > SYM_MAX_OPS) {
        conv_fail(a, b, lane, n, system, 0, find_status | SYM_CONV_FAIL, true);
        return;
    }
    const int* rot = a.sym_rot + (size_t)b * SYM_MAX_OPS * 9;
    for (int i = lane; i < nops; i += 64) {
        int W[9], order = -1, axis[3] = {0, 0, 0};
        bool fresh = i == 0;
#pragma unroll
        for (int e = 0; e < 9; ++e) W[e] = rot[9 * i + e], fresh = fresh || W[e] != rot[9 * (i > 0 ? i - 1 : 0) + e];
        if (fresh) conv_classify(W, &order, axis);
        s_order[i] = order, s_axis[3 * i] = axis[0], s_axis[3 * i + 1] = axis[1], s_axis[3 * i + 2] = axis[2];
    }
    __syncthreads();
    if (lane == 0) {
        conv_collect_begin(&s_ax);
        for (int i = 0; i < nops; ++i) conv_collect(&s_ax, i, s_order[i], s_axis + 3 * i);
    }
    __syncthreads();
    double L[9], G[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) L[i] = a.set.lat[(size_t)b * 9 + i];
    sym_metric(L, G);
    int M[9], n_axes = 0, mult = 1, centring = CONV_NONE, bravais = 0;
    int* cvec = s_cvec[lane];
    const ConvWaveSearch search{G, lane};
    if (conv_basis(system, s_ax, rot, G, CONV_BOX, search, M, &n_axes)) bravais = conv_finish(system, M, &mult, &centring, cvec);   // (uniform)
    int T[9], adj[9];
    double L0[9], Lr[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) L0[i] = (double)a.lat[(size_t)b * 9 + i];
    sm_reduce(L0, T, Lr);   // (the prepare status is OK: the reduction ended)
    if (bravais == 0 || !conv_transform(M, T, adj)) {
        conv_fail(a, b, lane, n, system, n_axes, find_status | SYM_CONV_FAIL, true);
        return;
    }
    const int row[CONV_INFO] = {bravais, centring, mult, system, n_axes, conv_max_abs(M), 0, find_status};
#pragma unroll
    for (int i = 0; i < CONV_INFO; ++i)
        if (lane == i) a.conv_info[(size_t)b * CONV_INFO + i] = row[i];
#pragma unroll
    for (int i = 0; i < 9; ++i)
        if (lane == i) a.conv_M[(size_t)b * 9 + i] = M[i], a.ws_adj[(size_t)b * 9 + i] = adj[i];
    if (lane < CONV_MAX_MULT * 3) a.conv_cvec[(size_t)b * CONV_MAX_MULT * 3 + lane] = cvec[lane];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double r[3];
        conv_lat_row(M, Lr, i, r);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (lane == 3 * i + c) a.out_lat[(size_t)b * 9 + 3 * i + c] = (float)r[c];
    }
    if (lane == 0) a.conv_count[b] = mult * n;
}

// conv_offsets [B + 1]: the running sum of conv_count, chunks of 256 crystals with a carried total
__global__ __launch_bounds__(SM_THREADS) void sym_conv_scan_kernel(const int* count, int* offsets, int B) {
    __shared__ int s_sum[2][SM_THREADS];
    const int tid = threadIdx.x;
    int carry = 0;
    if (tid == 0) offsets[0] = 0;
    for (int base = 0; base < B; base += SM_THREADS) {   // (uniform)
        int cur = 0;
        s_sum[cur][tid] = base + tid < B ? count[base + tid] : 0;
        __syncthreads();
        for (int d = 1; d < SM_THREADS; d <<= 1) {
            s_sum[cur ^ 1][tid] = s_sum[cur][tid] + (tid >= d ? s_sum[cur][tid - d] : 0);
            cur ^= 1;
            __syncthreads();
        }
        if (base + tid < B) offsets[base + tid + 1] = carry + s_sum[cur][tid];
        carry += s_sum[cur][SM_THREADS - 1];
        __syncthreads();   // the next chunk rewrites s_sum
    }
}

__global__ __launch_bounds__(SM_THREADS) void sym_conv_gather_kernel(mi_sym_conv_args a) {
    const int B = a.set.B;
    const int64_t t64 = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
    const int total = a.conv_offsets[B];
    if (t64 >= (int64_t)total || t64 >= (int64_t)4 * a.set.N) return;   // (offsets that overlap: the output arrays hold 4 N atoms)
    const int t = (int)t64;
    int lo = 0, hi = B - 1;   // the crystal b with conv_offsets[b] <= t < conv_offsets[b + 1]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.conv_offsets[mid + 1] > t) hi = mid;
        else lo = mid + 1;
    }
    const int b = lo, r = t - a.conv_offsets[b];
    const int* info = a.conv_info + (size_t)b * CONV_INFO;
    const int mult = info[2];
    const int n0 = a.set.offsets[b], n = a.set.info[(size_t)b * 4];   // (a crystal with atoms passed the prepare guard)
    if (r < 0 || mult < 1 || mult > CONV_MAX_MULT) return;
    const int i = r / mult, j = r - i * mult;
    if (i >= n) return;
    const float* f = a.frac + (size_t)(n0 + i) * 3;
    a.out_types[t] = a.types[n0 + i];
    if (info[0] == 0) {   // no basis: unchanged
#pragma unroll
        for (int c = 0; c < 3; ++c) a.out_frac[(size_t)t * 3 + c] = f[c];
        return;
    }
    int adj[9], v[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) adj[e] = a.ws_adj[(size_t)b * 9 + e];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = a.conv_cvec[((size_t)b * CONV_MAX_MULT + j) * 3 + c];
    float out[3];
    conv_frac(f, adj, v, mult, out);
#pragma unroll
    for (int c = 0; c < 3; ++c) a.out_frac[(size_t)t * 3 + c] = out[c];
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_sym_conventional(const mi_sym_conv_args* args, void* stream) {
    MI_CHECK(args, MI_EINVAL, "mi_sym_conventional: null argument block");
    const mi_sym_conv_args& a = *args;
    const mi_sm_prepared& s = a.set;
    MI_CHECK(s.B >= 0 && s.N >= 0, MI_EINVAL, "mi_sym_conventional: negative count (B %d, N %d)", s.B, s.N);
    if (s.B == 0) return MI_OK;
    MI_CHECK(s.N <= 0x7fffffff / 4, MI_EINVAL, "mi_sym_conventional: 4 N beyond int32 (N %d)", s.N);
    MI_CHECK(s.offsets && s.lat && s.inv && s.frac && s.types && s.perm && s.spec_Z && s.spec_off && s.info, MI_EINVAL,
             "mi_sym_conventional: null pointer in a prepared set");
    MI_CHECK(a.lat && a.sym_info && a.sym_rot && a.ws_adj && a.conv_info && a.conv_M && a.conv_cvec && a.conv_count && a.conv_offsets && a.out_lat, MI_EINVAL,
             "mi_sym_conventional: null pointer");
    MI_CHECK(s.N == 0 || (a.types && a.frac && a.out_types && a.out_frac), MI_EINVAL, "mi_sym_conventional: null atom array");
    hipLaunchKernelGGL(sym_conv_basis_kernel, dim3(s.B), dim3(64), 0, (hipStream_t)stream, a);
    MI_KERNEL_CHECK();
    hipLaunchKernelGGL(sym_conv_scan_kernel, dim3(1), dim3(SM_THREADS), 0, (hipStream_t)stream, (const int*)a.conv_count, a.conv_offsets, s.B);
    MI_KERNEL_CHECK();
    if (s.N > 0) {
        const int64_t threads = (int64_t)4 * s.N;
        hipLaunchKernelGGL(sym_conv_gather_kernel, dim3((unsigned)((threads + SM_THREADS - 1) / SM_THREADS)), dim3(SM_THREADS), 0, (hipStream_t)stream, a);
        MI_KERNEL_CHECK();
    }
    return MI_OK;
}

}  // extern "C"
