// Composition validity (include/matinvent_hip_chem.h).  Launches of this unit, 256 threads each, no atomics, no scratch, no matrix pipe:
//   chem_plan_kernel    one workgroup per crystal: the types checked, the atoms counted per Z bin (thread z - 1 owns bin z and strides over the
//                       atoms: no LDS atomics), one lane composes (gcd, status, N, chunk count) into the workspace;
//   chem_enum_kernel    a grid fixed on the host (<= CHEM_MAX_GRID workgroups): each workgroup scans the chunk counts of the batch into its
//                       own copy of the work-item table in LDS (item -> crystal by bisection, chunk by difference) and grid-strides over the
//                       items; per item the state table goes to LDS, every thread runs CHEM_RUN contiguous combinations, and the three
//                       partials are reduced through one fixed tree (xor butterfly inside a wave, then the four waves in order);
//   chem_reduce_kernel  one workgroup per crystal: its items folded in chunk order, every output written, atom_ox included.
// csrc/chem_enum.h holds every formula, host and device.

#include "../../include/matinvent_hip_chem.h"
#include "common.h"
#include "chem_enum.h"

namespace mi {

static_assert(CHEM_MAX_Z == MI_CHEM_MAX_Z && CHEM_MAX_STATES == MI_CHEM_MAX_STATES && CHEM_MAX_ELEMS == MI_CHEM_MAX_ELEMS && CHEM_CHUNK == MI_CHEM_CHUNK &&
                  CHEM_MAX_GRID == MI_CHEM_MAX_GRID && CHEM_MAX_BATCH == MI_CHEM_MAX_BATCH,
              "sizes");
static_assert(CHEM_ENUMERATED == MI_CHEM_ENUMERATED && CHEM_ELEMENTAL == MI_CHEM_ELEMENTAL && CHEM_ALLOY == MI_CHEM_ALLOY && CHEM_BAD_INPUT == MI_CHEM_BAD_INPUT &&
                  CHEM_TOO_MANY_ELEMENTS == MI_CHEM_TOO_MANY_ELEMENTS && CHEM_UNKNOWN_ELEMENT == MI_CHEM_UNKNOWN_ELEMENT && CHEM_NO_STATES == MI_CHEM_NO_STATES &&
                  CHEM_TOO_MANY_COMBOS == MI_CHEM_TOO_MANY_COMBOS,
              "status codes");
static_assert(CHEM_THREADS == CHEM_MAX_ELEMS * CHEM_MAX_STATES, "one thread per cell of an item's state table");
static_assert(CHEM_THREADS >= CHEM_MAX_Z, "one thread per Z bin");

struct ChemArgs {
    mi_chem_args a;
    ChemPlan* ws_plan;      // [B]
    int* ws_chunks;         // [B]
    int64_t* ws_partial;    // [items][3]: first (absolute, -1: none), neutral, passing
};

__device__ __forceinline__ ChemTable chem_table(const mi_chem_args& a) { return ChemTable{a.present, a.n_states, a.ox, a.eneg_rank, a.is_metal}; }

__global__ __launch_bounds__(CHEM_THREADS) void chem_plan_kernel(ChemArgs A) {
    __shared__ int cnt[CHEM_MAX_Z + 1];
    __shared__ ChemPlan plan;
    const mi_chem_args& a = A.a;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int o0 = a.node_off[b], o1 = a.node_off[b + 1];
    const bool range_ok = o0 >= 0 && o0 < o1 && o1 <= a.N;   // (uniform; o0 == o1: zero atoms)
    int bad = 0;
    if (range_ok)
        for (int i = o0 + tid; i < o1; i += CHEM_THREADS) bad |= !chem_type_ok(a.atom_types[i]);
    bad = __syncthreads_or(bad) || !range_ok;
    if (tid <= CHEM_MAX_Z) {
        int c = 0;
        if (!bad && tid >= 1)
            for (int i = o0; i < o1; ++i) c += a.atom_types[i] == tid;
        cnt[tid] = c;
    }
    __syncthreads();
    if (tid == 0) {
        chem_compose(cnt, bad != 0, chem_table(a), a.include_alloys, a.max_combos, plan);
        A.ws_chunks[b] = plan.n_chunks;
    }
    __syncthreads();
    int* dst = (int*)(A.ws_plan + b);
    const int* src = (const int*)&plan;
    for (int i = tid; i < (int)(sizeof(ChemPlan) / sizeof(int)); i += CHEM_THREADS) dst[i] = src[i];
}

// Inclusive scan of one value per thread over the workgroup; `tot` receives the workgroup's sum.  red: [CHEM_THREADS / 64] ints.
__device__ __forceinline__ int chem_block_scan(int v, int* red, int tid, int& tot) {
    const int lane = tid & 63;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int o = __shfl_up(v, m, 64);
        if (lane >= m) v += o;
    }
    if (lane == 63) red[tid >> 6] = v;
    __syncthreads();
    int base = 0;
    tot = 0;
#pragma unroll
    for (int w = 0; w < CHEM_THREADS / 64; ++w) {
        if (w < (tid >> 6)) base += red[w];
        tot += red[w];
    }
    __syncthreads();
    return v + base;
}

__global__ __launch_bounds__(CHEM_THREADS) void chem_enum_kernel(ChemArgs A) {
    __shared__ int item_off[CHEM_MAX_BATCH + 1];   // the work-item table: crystal b owns the items item_off[b] .. item_off[b + 1] - 1
    __shared__ ChemItem item;
    __shared__ ChemPlan plan;
    __shared__ int red[3][CHEM_THREADS / 64];
    const mi_chem_args& a = A.a;
    const int tid = threadIdx.x;
    const ChemTable T = chem_table(a);
    int running = 0;
    for (int b0 = 0; b0 < a.B; b0 += CHEM_THREADS) {   // (uniform)
        const int b = b0 + tid;
        int tot;
        const int inc = chem_block_scan(b < a.B ? A.ws_chunks[b] : 0, red[0], tid, tot);
        if (b < a.B) item_off[b + 1] = running + inc;
        running += tot;
    }
    if (tid == 0) item_off[0] = 0;
    __syncthreads();
    const int n_items = item_off[a.B];
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {   // (uniform)
        int lo = 0, hi = a.B;   // the crystal whose range holds `it`: item_off[lo] <= it < item_off[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (item_off[mid] <= it) lo = mid;
            else hi = mid;
        }
        const int chunk = it - item_off[lo];
        {
            int* dst = (int*)&plan;
            const int* src = (const int*)(A.ws_plan + lo);
            for (int i = tid; i < (int)(sizeof(ChemPlan) / sizeof(int)); i += CHEM_THREADS) dst[i] = src[i];
        }
        __syncthreads();
        {
            const int pos = tid / CHEM_MAX_STATES, s = tid % CHEM_MAX_STATES;
            chem_item_cell(plan, T, pos, s, item.ox[pos][s], item.w[pos][s]);
            if (tid < CHEM_MAX_ELEMS) chem_item_head(plan, tid, item.radix[tid], item.rank[tid]);
        }
        __syncthreads();
        const int64_t c0 = (int64_t)chunk * CHEM_CHUNK;
        const int64_t left = plan.n_combos - c0 - (int64_t)tid * CHEM_RUN;   // combinations from this thread's start to N
        int first_rel = CHEM_NO_FIRST, nn = 0, nv = 0;
        if (left > 0) {
            chem_run(item, c0 + (int64_t)tid * CHEM_RUN, left < CHEM_RUN ? (int)left : CHEM_RUN, a.use_pauling_test, plan.any_unranked, first_rel, nn, nv);
            if (first_rel != CHEM_NO_FIRST) first_rel += tid * CHEM_RUN;   // relative to the chunk: below 65536
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const int of = __shfl_xor(first_rel, m, 64);
            first_rel = of < first_rel ? of : first_rel;
            nn += __shfl_xor(nn, m, 64);
            nv += __shfl_xor(nv, m, 64);
        }
        if ((tid & 63) == 0) red[0][tid >> 6] = first_rel, red[1][tid >> 6] = nn, red[2][tid >> 6] = nv;
        __syncthreads();
        if (tid == 0) {
            int f = red[0][0], n1 = red[1][0], n2 = red[2][0];
#pragma unroll
            for (int w = 1; w < CHEM_THREADS / 64; ++w) {
                f = red[0][w] < f ? red[0][w] : f;
                n1 += red[1][w];
                n2 += red[2][w];
            }
            int64_t* out = A.ws_partial + (size_t)it * 3;
            out[0] = f == CHEM_NO_FIRST ? -1 : c0 + f;
            out[1] = n1;
            out[2] = n2;
        }
        __syncthreads();   // red, plan and item are rewritten by the next item
    }
}

__global__ __launch_bounds__(CHEM_THREADS) void chem_reduce_kernel(ChemArgs A) {
    __shared__ ChemPlan plan;
    __shared__ int64_t tree[3][CHEM_THREADS];
    __shared__ int red[CHEM_THREADS / 64];
    __shared__ int first_ox[CHEM_MAX_ELEMS];
    const mi_chem_args& a = A.a;
    const int b = blockIdx.x, tid = threadIdx.x;
    const ChemTable T = chem_table(a);
    {
        int* dst = (int*)&plan;
        const int* src = (const int*)(A.ws_plan + b);
        for (int i = tid; i < (int)(sizeof(ChemPlan) / sizeof(int)); i += CHEM_THREADS) dst[i] = src[i];
    }
    int before = 0;   // the items of the crystals before this one
    for (int j = tid; j < b; j += CHEM_THREADS) before += A.ws_chunks[j];
    int item0;
    chem_block_scan(before, red, tid, item0);   // (its barriers also publish `plan`)
    // thread t folds chunks t, t + 256, ... in ascending order; the tree below then joins neighbours, lower chunks on the left
    int64_t first = -1, nn = 0, nv = 0;
    for (int c = tid; c < plan.n_chunks; c += CHEM_THREADS) {
        const int64_t* p = A.ws_partial + (size_t)(item0 + c) * 3;
        chem_fold(first, nn, nv, p[0], p[1], p[2]);
    }
    tree[0][tid] = first, tree[1][tid] = nn, tree[2][tid] = nv;
    __syncthreads();
    for (int m = CHEM_THREADS / 2; m >= 1; m >>= 1) {
        if (tid < m) chem_fold(tree[0][tid], tree[1][tid], tree[2][tid], tree[0][tid + m], tree[1][tid + m], tree[2][tid + m]);
        __syncthreads();
    }
    first = tree[0][0], nn = tree[1][0], nv = tree[2][0];
    if (tid == 0) chem_first_states(plan, T, first, first_ox);
    __syncthreads();
    if (tid < CHEM_MAX_ELEMS) {
        a.elems[(size_t)b * CHEM_MAX_ELEMS + tid] = plan.elems[tid];
        a.counts[(size_t)b * CHEM_MAX_ELEMS + tid] = plan.counts[tid];
        a.first_ox[(size_t)b * CHEM_MAX_ELEMS + tid] = first_ox[tid];
    }
    if (tid == 0) {
        a.valid[b] = chem_valid(plan.status, nv) ? 1 : 0;
        a.status[b] = plan.status;
        a.n_elems[b] = plan.n_elems;
        a.n_combos[b] = plan.n_combos;
        a.n_neutral[b] = nn;
        a.n_valid[b] = nv;
        a.first[b] = first;
    }
    const int o0 = a.node_off[b], o1 = a.node_off[b + 1];
    if (!(o0 >= 0 && o0 < o1 && o1 <= a.N)) return;   // (uniform) no atom rows
    for (int i = o0 + tid; i < o1; i += CHEM_THREADS) a.atom_ox[i] = plan.status == CHEM_ENUMERATED ? chem_atom_state(plan, first_ox, a.atom_types[i]) : 0;
}

static int64_t chem_align16(int64_t n) { return (n + 15) / 16 * 16; }

// the largest number of work items that B crystals under the cap can have; -1: not representable
static int64_t chem_max_items(int B, int64_t max_combos) {
    if (B < 0 || B > CHEM_MAX_BATCH || max_combos < 1 || max_combos > CHEM_COMBOS_CAP) return -1;
    const int64_t items = (int64_t)B * ((max_combos + CHEM_CHUNK - 1) / CHEM_CHUNK);
    return items > 0x7fffffffLL ? -1 : items;
}

static int chem_launch(const mi_chem_args* args, hipStream_t stream) {
    MI_CHECK(args, MI_EINVAL, "chem: null argument block");
    const mi_chem_args& a = *args;
    MI_CHECK(a.B >= 0 && a.N >= 0, MI_EINVAL, "chem: negative count (B %d, N %d)", a.B, a.N);
    MI_CHECK(a.B <= CHEM_MAX_BATCH, MI_EINVAL, "chem: B = %d beyond %d crystals per call", a.B, CHEM_MAX_BATCH);
    MI_CHECK(a.max_combos >= 1 && a.max_combos <= CHEM_COMBOS_CAP, MI_EINVAL, "chem: max_combos = %lld outside 1..32^8", (long long)a.max_combos);
    const int64_t items = chem_max_items(a.B, a.max_combos);
    MI_CHECK(items >= 0, MI_EINVAL, "chem: B = %d under max_combos = %lld is more than 2^31 - 1 work items", a.B, (long long)a.max_combos);
    MI_CHECK(a.valid && a.status && a.n_elems && a.elems && a.counts && a.n_combos && a.n_neutral && a.n_valid && a.first && a.first_ox && a.atom_ox, MI_EINVAL,
             "chem: null output pointer");
    MI_CHECK(a.present && a.n_states && a.ox && a.eneg_rank && a.is_metal && a.node_off && a.atom_types && a.workspace, MI_EINVAL, "chem: null input pointer");
    MI_CHECK(((uintptr_t)a.workspace & 15) == 0, MI_EINVAL, "chem: the workspace must be 16-byte aligned");
    if (a.B == 0) return MI_OK;
    ChemArgs A;
    A.a = a;
    char* w = (char*)a.workspace;
    A.ws_plan = (ChemPlan*)w;
    w += chem_align16((int64_t)a.B * (int64_t)sizeof(ChemPlan));
    A.ws_chunks = (int*)w;
    w += chem_align16((int64_t)a.B * (int64_t)sizeof(int));
    A.ws_partial = (int64_t*)w;
    const int grid = (int)(items < CHEM_MAX_GRID ? items : CHEM_MAX_GRID);   // from B and max_combos, never from device data
    hipLaunchKernelGGL(chem_plan_kernel, dim3(a.B), dim3(CHEM_THREADS), 0, stream, A);
    MI_KERNEL_CHECK();
    hipLaunchKernelGGL(chem_enum_kernel, dim3(grid), dim3(CHEM_THREADS), 0, stream, A);
    MI_KERNEL_CHECK();
    hipLaunchKernelGGL(chem_reduce_kernel, dim3(a.B), dim3(CHEM_THREADS), 0, stream, A);
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int64_t mi_chem_workspace(int B, int64_t max_combos) {
    const int64_t items = chem_max_items(B, max_combos);
    MI_CHECK(items >= 0, MI_EINVAL, "chem workspace: B = %d outside 0..%d, max_combos = %lld outside 1..32^8, or more than 2^31 - 1 work items", B, CHEM_MAX_BATCH,
             (long long)max_combos);
    return chem_align16((int64_t)B * (int64_t)sizeof(ChemPlan)) + chem_align16((int64_t)B * (int64_t)sizeof(int)) + chem_align16(items * 3 * (int64_t)sizeof(int64_t)) + 16;
}

int mi_chem_validity(const mi_chem_args* args, void* stream) { return chem_launch(args, (hipStream_t)stream); }

}  // extern "C"
