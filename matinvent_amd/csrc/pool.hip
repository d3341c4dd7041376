// A device-memory pool for batch handles and the index-table kernels of a pooled handle (include/matinvent_hip_pool.h).
//
// The pool keeps hipMalloc'd blocks of a few size classes.  A pooled handle asks for each of its exact-size buffers through dev_alloc
// (cspnet.hip); the request takes the smallest cached block whose class is at least the request's class -- whatever that block was used
// for before -- or a fresh hipMalloc of the class.  mi_batch_destroy hands the blocks back; nothing is freed until mi_pool_trim,
// mi_pool_destroy, or a request that would exceed the cap.  Reuse is ordered by the pool's ONE stream: the releasing handle's work and
// the next handle's set-up and work are all enqueued there, so a block may change hands without a wait.
//
// Typed hand-out.  Blocks of int / unsigned elements (index tables, arrival counters, absmax slots) are ALWAYS zero-filled on the pool's
// stream, fresh or recycled: a stale value there would be an out-of-range index or a counter that never reaches its target.  Blocks of
// float / fp16-plane elements are handed out as they are; with poison on, pool_poison_kernel fills them with quiet NaN first, so that a
// buffer that relied on fresh pages being zero shows as NaN instead of passing by luck.
//
// Kernels of this unit:
//   pool_poison_kernel         16-byte vector stores of one 32-bit pattern over a block (grid-stride);
//   pool_crystal_node_kernel   one thread per crystal (num_atoms) and per node + 1 (node2graph, rowptr, e_diag);
//   pool_edge_kernel           one thread per edge (src, dst, edge_graph);
//   pool_pair_kernel           one thread per unordered pair (pair_i, pair_j, pair_e1, pair_e2, pair_graph).
// The decode is csrc/pool_tables.h, compiled for the host as well by scripts/pool_tables_host_check.cpp.
#include <map>
#include <mutex>
#include <unordered_map>

#include "../../include/matinvent_hip_pool.h"
#include "net.h"
#include "pool_tables.h"

struct mi_pool {
    hipStream_t stream = nullptr;
    int64_t max_bytes = 0;   // 0: no cap
    int poison = 0;
    mutable std::mutex mu;
    std::multimap<size_t, void*> cached;          // class bytes -> block, unused
    std::unordered_map<void*, size_t> lent;       // block -> class bytes, held by a handle
    int64_t reserved = 0, in_use = 0, n_malloc = 0, n_hit = 0, n_free = 0, live = 0, high = 0;
};

namespace mi {

static size_t pool_class(size_t request) {
    size_t c = 512;
    if (request <= ((size_t)1 << 20)) {
        while (c < request) c <<= 1;
        return c;
    }
    size_t p = (size_t)1 << 20;   // the power of two that encloses the request from below: p <= request < 2 p
    while (p * 2 <= request) p <<= 1;
    const size_t step = p >> 3;   // (the class exceeds the request by less than p / 8 <= request / 8)
    return (request + step - 1) / step * step;
}

// n16 16-byte words at p (a block of the pool: its class is a multiple of 512 bytes and hipMalloc aligns it to 256)
__global__ __launch_bounds__(256) void pool_poison_kernel(uint4* __restrict__ p, size_t n16, unsigned pattern) {
    const uint4 v = make_uint4(pattern, pattern, pattern, pattern);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

__global__ __launch_bounds__(256) void pool_crystal_node_kernel(PoolTables t, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < t.B) pt_crystal(t, i);
    if (i <= N) pt_node(t, i);
}

__global__ __launch_bounds__(256) void pool_edge_kernel(PoolTables t, int64_t E) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E) pt_edge(t, e);
}

__global__ __launch_bounds__(256) void pool_pair_kernel(PoolTables t, int64_t Np) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < Np) pt_pair(t, p);
}

hipStream_t pool_stream(const mi_pool* pool) { return pool->stream; }

void pool_handle_count(mi_pool* pool, int delta) {
    std::lock_guard<std::mutex> g(pool->mu);
    pool->live += delta;
}

// hipFree of every cached block (the caller holds the mutex).  A cached block may still be read or written by work in flight on the
// pool's stream, and the runtime's own wait inside hipFree is not something to rest on: wait for the stream first.
static int pool_trim_locked(mi_pool* pool) {
    if (pool->cached.empty()) return MI_OK;
    MI_HIP(hipStreamSynchronize(pool->stream));
    for (auto& kv : pool->cached) {
        (void)hipFree(kv.second);
        pool->reserved -= (int64_t)kv.first;
        ++pool->n_free;
    }
    pool->cached.clear();
    return MI_OK;
}

int pool_alloc(mi_pool* pool, size_t bytes, int kind, void** out) {
    std::lock_guard<std::mutex> g(pool->mu);
    const size_t cls = pool_class(bytes);
    void* q = nullptr;
    size_t got = 0;
    auto it = pool->cached.lower_bound(cls);   // best fit: the smallest cached block that is large enough
    if (it != pool->cached.end()) {
        got = it->first;
        q = it->second;
        pool->cached.erase(it);
        ++pool->n_hit;
    } else {
        if (pool->max_bytes > 0 && pool->reserved + (int64_t)cls > pool->max_bytes) MI_TRY(pool_trim_locked(pool));
        if (pool->max_bytes > 0 && pool->reserved + (int64_t)cls > pool->max_bytes) {
            set_error("handle pool: a block of %zu bytes on top of %lld bytes in use exceeds the cap of %lld bytes", cls, (long long)pool->in_use,
                      (long long)pool->max_bytes);
            return MI_ENOMEM;
        }
        hipError_t e = hipMalloc(&q, cls);
        if (e != hipSuccess && !pool->cached.empty()) {   // the device is full: give the cached blocks back and ask once more
            (void)hipGetLastError();
            MI_TRY(pool_trim_locked(pool));
            e = hipMalloc(&q, cls);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error("handle pool: hipMalloc(%zu bytes) failed: %s", cls, hipGetErrorString(e));
            return MI_ENOMEM;
        }
        got = cls;
        ++pool->n_malloc;
        pool->reserved += (int64_t)cls;
    }
    pool->lent.emplace(q, got);
    pool->in_use += (int64_t)got;
    pool->high = std::max(pool->high, pool->in_use);
    *out = q;
    // the typed hand-out (see the head of this file), over the WHOLE block, on the pool's stream
    hipError_t e = hipSuccess;
    if (kind == POOL_INT) {
        e = hipMemsetAsync(q, 0, got, pool->stream);
    } else if (pool->poison) {
        const size_t n16 = got / 16;
        const unsigned pattern = kind == POOL_F32 ? 0x7FC00000u : 0x7E007E00u;
        const unsigned grid = (unsigned)std::min<size_t>((n16 + 255) / 256, 4096);
        hipLaunchKernelGGL(pool_poison_kernel, dim3(grid), dim3(256), 0, pool->stream, (uint4*)q, n16, pattern);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {   // (the block stays lent: the caller's handle holds it in `allocs` only after MI_OK, so hand it back here)
        pool->lent.erase(q);
        pool->in_use -= (int64_t)got;
        pool->cached.emplace(got, q);
        set_error("handle pool: filling a block failed: %s", hipGetErrorString(e));
        return MI_EHIP;
    }
    return MI_OK;
}

void pool_release(mi_pool* pool, void* p) {
    std::lock_guard<std::mutex> g(pool->mu);
    auto it = pool->lent.find(p);
    if (it == pool->lent.end()) return;
    pool->in_use -= (int64_t)it->second;
    pool->cached.emplace(it->second, p);
    pool->lent.erase(it);
}

int pool_build_tables(mi_batch* b, hipStream_t s) {
    PoolTables t{b->node_off, b->edge_off, b->pair_off, b->B, b->num_atoms, b->node2graph, b->rowptr, b->e_diag,
                 b->src,      b->dst,      b->edge_graph, b->pair_i, b->pair_j, b->pair_e1, b->pair_e2, b->pair_graph};
    const int N = b->N;
    const int64_t E = b->E, Np = b->Np;
    if (b->B > 0) {   // (B = 0: rowptr[0] = 0 is the block's zero fill)
        hipLaunchKernelGGL(pool_crystal_node_kernel, dim3(cdiv((int64_t)std::max(N + 1, b->B), 256)), dim3(256), 0, s, t, N);
        if (E > 0) hipLaunchKernelGGL(pool_edge_kernel, dim3((unsigned)cdiv(E, 256)), dim3(256), 0, s, t, E);
        if (Np > 0) hipLaunchKernelGGL(pool_pair_kernel, dim3((unsigned)cdiv(Np, 256)), dim3(256), 0, s, t, Np);
    }
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_pool_create(void* stream, int64_t max_bytes, mi_pool** out) {
    MI_CHECK(out, MI_EINVAL, "mi_pool_create: null argument");
    int dev = 0;
    MI_HIP(hipGetDevice(&dev));   // (no device: the library's error, not a pool that fails at its first request)
    mi_pool* p = new mi_pool();
    p->stream = (hipStream_t)stream;
    p->max_bytes = max_bytes > 0 ? max_bytes : 0;
    *out = p;
    return MI_OK;
}

int mi_pool_destroy(mi_pool* pool) {
    if (!pool) return MI_OK;
    {
        std::lock_guard<std::mutex> g(pool->mu);
        MI_CHECK(pool->live == 0 && pool->lent.empty(), MI_ESTATE, "mi_pool_destroy: %lld batch handle(s) created in this pool are alive",
                 (long long)pool->live);
        MI_TRY(pool_trim_locked(pool));
    }
    delete pool;
    return MI_OK;
}

int mi_pool_trim(mi_pool* pool) {
    MI_CHECK(pool, MI_EINVAL, "mi_pool_trim: null pool");
    std::lock_guard<std::mutex> g(pool->mu);
    return pool_trim_locked(pool);
}

int mi_pool_stats(const mi_pool* pool, int64_t out_host[8]) {
    MI_CHECK(pool && out_host, MI_EINVAL, "mi_pool_stats: null argument");
    std::lock_guard<std::mutex> g(pool->mu);
    out_host[0] = pool->reserved;
    out_host[1] = pool->in_use;
    out_host[2] = pool->n_malloc;
    out_host[3] = pool->n_hit;
    out_host[4] = pool->n_free;
    out_host[5] = pool->live;
    out_host[6] = pool->high;
    out_host[7] = pool->max_bytes;
    return MI_OK;
}

int64_t mi_pool_block_bytes(int64_t request) { return (int64_t)pool_class(request > 0 ? (size_t)request : 1); }

int mi_pool_set_poison(mi_pool* pool, int on) {
    MI_CHECK(pool, MI_EINVAL, "mi_pool_set_poison: null pool");
    std::lock_guard<std::mutex> g(pool->mu);
    pool->poison = on != 0;
    return MI_OK;
}

}  // extern "C"
