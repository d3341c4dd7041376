// Fingerprint matching (include/matinvent_hip_match.h): one 256-thread block per work item (a tile of 8 query rows x a chunk of
// candidates).  The tile sits in LDS, sized by the call's widest group; each wave carries 4 bank rows at a time past it, 16 bytes per lane and
// row, 32 fp32 FMA chains per lane, and folds them with a halving butterfly.  A second kernel folds each query's partials in chunk order.
// The body lives in fp_match_body.h, phase by phase, so that the host can run the same source.
#include "fp_match_body.h"
#include "common.h"

namespace mi {

template <int HALF>
__device__ __forceinline__ void fpm_level(FpmLane& r, int lane, int mask) {
    constexpr int N = HALF ? HALF : 1;
    float send[N], recv[N];
    fpm_level_send(r, lane, mask, HALF, send);
#pragma unroll
    for (int j = 0; j < N; ++j) recv[j] = __shfl_xor(send[j], mask, FPM_WAVE);
    fpm_level_add(r, lane, mask, HALF, recv);
}

__global__ __launch_bounds__(FPM_THREADS) void fp_match_kernel(FpmArgs A) {
    extern __shared__ __attribute__((aligned(16))) float fpm_tile[];
    __shared__ FpmShared s;
    const int tid = threadIdx.x, lane = tid % FPM_WAVE;
    fpm_phase_item(s, A, blockIdx.x, tid);
    __syncthreads();
    fpm_phase_stage(s, A, fpm_tile, tid);
    __syncthreads();
    if (!s.ok) return;
    FpmLane r;
    fpm_lane_init(r);
    const int passes = (s.c1 - s.c0 + FPM_PASS - 1) / FPM_PASS;
    for (int pass = 0; pass < passes; ++pass) {
        fpm_pass_accumulate(s, A, fpm_tile, tid, pass, r);
        fpm_level<16>(r, lane, 32);
        fpm_level<8>(r, lane, 16);
        fpm_level<4>(r, lane, 8);
        fpm_level<2>(r, lane, 4);
        fpm_level<1>(r, lane, 2);
        fpm_level<0>(r, lane, 1);
        fpm_pass_update(s, A, tid, pass, r);
    }
    fpm_phase_wave_out(s, tid, r);
    __syncthreads();
    fpm_phase_wave_status(s, tid, r);
    __syncthreads();
    fpm_phase_partial(s, A, tid);
}

__global__ __launch_bounds__(FPM_THREADS) void fp_match_reduce_kernel(FpmArgs A) {
    fpm_reduce_query(A, blockIdx.x * FPM_THREADS + threadIdx.x);
}

static bool fpm_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int fp_match_launch(const mi_fp_match_args* args, hipStream_t stream) {
    MI_CHECK(args, MI_EINVAL, "fp match: null argument block");
    const mi_fp_match_args& a = *args;
    MI_CHECK(a.Q >= 0 && a.M >= 0 && a.G >= 0 && a.nnz_q >= 0 && a.nnz_c >= 0 && a.n_items >= 0 && a.n_partials >= 0 && a.bank_floats >= 0 &&
                 a.pair_floats >= 0 && a.row_stride >= 0,
             MI_EINVAL, "fp match: negative count (Q %d, M %d, G %d, nnz_q %d, nnz_c %d, items %d, partials %d)", a.Q, a.M, a.G, a.nnz_q, a.nnz_c,
             a.n_items, a.n_partials);
    MI_CHECK(std::isfinite(a.tol) && a.tol >= 0.f && a.tol <= 1.f, MI_EINVAL, "fp match: tol = %g outside [0, 1]", (double)a.tol);
    MI_CHECK(a.row_stride % 4 == 0, MI_EINVAL, "fp match: row_stride = %d is not a multiple of 4 floats (16-byte loads)", a.row_stride);
    MI_CHECK(a.best_dist && a.best_idx && a.n_within && a.status, MI_EINVAL, "fp match: null output pointer");
    MI_CHECK(a.query && a.bank && a.bank_start && a.bank_len && a.grp_q_off && a.q_idx && a.grp_c_off && a.c_idx && a.grp_ncols && a.items &&
                 a.grp_part_off && a.workspace,
             MI_EINVAL, "fp match: null input pointer");
    MI_CHECK(!a.pair_dist || a.pair_off, MI_EINVAL, "fp match: pair_dist without pair_off");
    MI_CHECK(fpm_aligned16(a.query) && fpm_aligned16(a.bank) && fpm_aligned16(a.workspace), MI_EINVAL,
             "fp match: query, bank and workspace must be 16-byte aligned");
    MI_CHECK(a.max_ncols >= 1 && a.max_ncols <= FPM_MAX_LEN, MI_EINVAL, "fp match: max_ncols = %d outside 1..%d", a.max_ncols, FPM_MAX_LEN);
    if (a.G == 0 || a.Q == 0 || a.nnz_q == 0) return MI_OK;
    FpmArgs A;
    A.a = a;
    const size_t n = (size_t)a.n_partials;
    A.part_dist = (float*)a.workspace;
    A.part_idx = (int*)a.workspace + n;
    A.part_cnt = (int*)a.workspace + 2 * n;
    A.part_status = (int*)a.workspace + 3 * n;
    if (n) MI_HIP(hipMemsetAsync(A.part_status, 0xFF, n * sizeof(int), stream));   // FPM_UNWRITTEN: a rejected item's partials stay marked
    if (a.n_items > 0) {
        const size_t lds = (size_t)FPM_TQ * fpm_round4(a.max_ncols) * sizeof(float);
        hipLaunchKernelGGL(fp_match_kernel, dim3(a.n_items), dim3(FPM_THREADS), lds, stream, A);
        MI_KERNEL_CHECK();
    }
    hipLaunchKernelGGL(fp_match_reduce_kernel, dim3((a.nnz_q + FPM_THREADS - 1) / FPM_THREADS), dim3(FPM_THREADS), 0, stream, A);
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_fp_match_plan(const int* grp_q_off_host, const int* grp_c_off_host, int G, int chunk, int* items_host, int* grp_part_off_host,
                     int64_t* n_items, int64_t* n_partials) {
    const int used = fpm_plan(grp_q_off_host, grp_c_off_host, G, chunk, items_host, grp_part_off_host, n_items, n_partials);
    MI_CHECK(used > 0, MI_EINVAL, "fp match plan: null array, G = %d < 0, decreasing offsets, or too many work items", G);
    return used;
}

int64_t mi_fp_match_workspace(int64_t n_partials) {
    MI_CHECK(n_partials >= 0, MI_EINVAL, "fp match workspace: n_partials = %lld < 0", (long long)n_partials);
    return 16 * (n_partials > 0 ? n_partials : 1);
}

int mi_fp_match(const mi_fp_match_args* args, void* stream) { return fp_match_launch(args, (hipStream_t)stream); }

}  // extern "C"
