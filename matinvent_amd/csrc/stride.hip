// Strided reverse chains (include/matinvent_hip_stride.h): a batch handle's step-index -> trained-time map and the time
// embedding that reads it.  Everything else of a strided chain is the full chain's code on shorter tables.
//
// The embedding's arithmetic is time_embedding_kernel's (sampler.hip), separately rounded: no contraction here either.
#pragma clang fp contract(off)

#include "../../include/matinvent_hip_stride.h"
#include "net.h"

namespace mi {

// out[b] = [sin(map[k_b] f_c) | cos(map[k_b] f_c)], k_b = steps[b], or k_all for every crystal when steps == NULL (the sampler's step).
// One thread per output element.  k is clamped to the map (the callers have checked it on the host; a stray index must not read outside).
__global__ void time_embedding_mapped_kernel(const int* __restrict__ map, int n, const int* __restrict__ steps, const float* __restrict__ freqs,
                                             float* __restrict__ out, int B, int TD, int k_all) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)B * TD) return;
    const int b = (int)(idx / TD), c = (int)(idx % TD), half = TD / 2;
    int k = steps ? steps[b] : k_all;
    k = k < 0 ? 0 : (k >= n ? n - 1 : k);
    const float arg = (float)map[k] * freqs[c < half ? c : c - half];
    out[idx] = c < half ? sinf(arg) : cosf(arg);
}

int time_embedding_mapped(const mi_batch* b, const int* steps, int k_all, const float* freqs, int B, int TD, float* out, hipStream_t s) {
    MI_CHECK(b && b->time_map && freqs && out && TD % 2 == 0, MI_EINVAL, "bad argument");
    if (B <= 0) return MI_OK;
    hipLaunchKernelGGL(time_embedding_mapped_kernel, dim3(cdiv((int64_t)B * TD, 256)), dim3(256), 0, s, (const int*)b->time_map,
                       (int)b->time_map_h.size(), steps, freqs, out, B, TD, k_all);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int time_map_check(const mi_batch* b, int T, const char* what) {
    MI_CHECK(!b->time_map || (int)b->time_map_h.size() == T + 1, MI_EINVAL, "%s carries a time map of %d entries, the call has T + 1 = %d", what,
             (int)b->time_map_h.size(), T + 1);
    return MI_OK;
}

int time_map_same(const mi_batch* p, const mi_batch* q, const char* what) {
    MI_CHECK((p->time_map != nullptr) == (q->time_map != nullptr) && p->time_map_h == q->time_map_h, MI_EINVAL, "%s", what);
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_batch_set_time_map(mi_batch* b, const int* map_host, int n) {
    MI_NO_POOLED(b, "mi_batch_set_time_map");
    MI_CHECK(b, MI_EINVAL, "null handle");
    MI_CHECK(n >= 0, MI_EINVAL, "n = %d: must be >= 0", n);
    if (n == 0) {
        b->time_map = nullptr;
        b->time_map_h.clear();
        return MI_OK;
    }
    MI_CHECK(map_host && n >= 2, MI_EINVAL, "a time map needs at least two entries (n = %d)", n);
    MI_CHECK(map_host[0] == 0, MI_EINVAL, "time map: map[0] = %d, must be 0", map_host[0]);
    for (int k = 1; k < n; ++k)
        MI_CHECK(map_host[k] > map_host[k - 1], MI_EINVAL, "time map: map[%d] = %d is not above map[%d] = %d (strictly increasing)", k, map_host[k],
                 k - 1, map_host[k - 1]);
    if (n > b->time_map_cap) {
        MI_TRY(dev_alloc(b, &b->time_map_buf, (size_t)n));
        b->time_map_cap = n;
    }
    MI_HIP(hipMemcpy(b->time_map_buf, map_host, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    b->time_map = b->time_map_buf;
    b->time_map_h.assign(map_host, map_host + n);
    return MI_OK;
}

}  // extern "C"
