// What the units that differentiate a learned energy by finite differences share on the device (vib.hip, elastic.hip, phonon.hip):
// the plan entry of a chunk's copy, the copy of its source crystal's type rows, and the block maximum of the asymmetry measures.  No
// formula lives here: those are in the __host__ __device__ headers (vib_dynmat.h, elastic_fit.h, phonon_fc.h), pinned by their restatements.
#pragma once
#include "common.h"

namespace mi {

constexpr int TYPE_COLS = 100;   // the type rows' width (matinvent_hip_scalar.h): 25 float4

// the plan entry of copy k of a chunk: its source crystal, copy index, atom count n and the first atom of the source (s0) and of the copy (c0).
// A crystal of n atoms has copies_per_atom * n + copies_fixed copies and at most max_atoms atoms.  false: the entry is not admissible
// (uniform over the workgroup), and nothing may be addressed through it.
__device__ __forceinline__ bool chunk_plan_entry(const int* plan_src, const int* plan_copy, int Bs, const int* src_node_off, const int* node_off, int k,
                                                 int copies_per_atom, int copies_fixed, int max_atoms, int* src, int* c, int* n, int* s0, int* c0) {
    *src = plan_src[k], *c = plan_copy[k];
    if (*src < 0 || *src >= Bs) return false;
    *s0 = src_node_off[*src];
    *n = src_node_off[*src + 1] - *s0;
    *c0 = node_off[k];
    return *n >= 1 && *n <= max_atoms && node_off[k + 1] - *c0 == *n && *c >= 0 && *c < copies_per_atom * *n + copies_fixed;
}

// the n type rows of the source crystal at atom s0 into the copy at atom c0, as float4 (both arrays 16-byte aligned: the entries check)
__device__ __forceinline__ void chunk_copy_types(const float* src_types, float* types, int s0, int c0, int n, int tid, int threads) {
    const float4* ts = reinterpret_cast<const float4*>(src_types + (size_t)s0 * TYPE_COLS);
    float4* td = reinterpret_cast<float4*>(types + (size_t)c0 * TYPE_COLS);
    for (int i = tid; i < n * (TYPE_COLS / 4); i += threads) td[i] = ts[i];
}

// the maximum of v (finite, >= 0) over a block of THREADS threads, red [THREADS / 64]: exact, so no order to fix
template <int THREADS>
__device__ __forceinline__ double block_max_f64(double v, double* red, int tid) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double o = __shfl_xor(v, m, 64);
        v = o > v ? o : v;
    }
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    v = red[0];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) v = red[w] > v ? red[w] : v;
    return v;
}

}  // namespace mi
