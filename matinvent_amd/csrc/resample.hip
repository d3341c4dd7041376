// Resampling jumps for the conditioned reverse chain (include/matinvent_hip_resample.h): a batch handle's (r, j) and jump
// table, the schedule of visited levels, the per-visit seed and the one kernel that jumps a state j noise levels forward.
//
// The arithmetic is the forward process between two levels, separately rounded like condition_impose_kernel's: no contraction here either.
#pragma clang fp contract(off)

#include <cmath>

#include "../../include/matinvent_hip_resample.h"
#include "net.h"

namespace mi {

struct JumpArgs {
    const float* table;        // [levels][3] = (c0, c1, s) of the jump a -> a + j
    const int* node_off;       // [B + 1]
    float *atom_types, *frac, *lattices;   // the state, every element updated in place
    uint64_t seed;
    int64_t node_offset, graph_offset;
    int from, to;
};

// One 256-thread block per crystal, in the shape of condition_impose_kernel: the lattice on threads 0..8, the coordinates strided over
// the block, the type rows one wave per atom with a lane owning a quad of logits = one Philox call.  Every element is read, drawn for
// and written: a jump knows no mask.
__global__ __launch_bounds__(256) void resample_jump_kernel(JumpArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t to = (uint32_t)a.to;
    const float c0 = a.table[a.from * 3 + 0], c1 = a.table[a.from * 3 + 1], sj = a.table[a.from * 3 + 2];
    const int n0 = a.node_off[b], n1 = a.node_off[b + 1];

    // lattice: l = c0 l + c1 z
    if (tid < 9) {
        const int idx = b * 9 + tid;
        const float z = philox_normal1(a.seed, to, DRAW_JUMP_L, (uint64_t)a.graph_offset * 9 + idx);
        a.lattices[idx] = c0 * a.lattices[idx] + c1 * z;
    }

    // coordinates: x = (x + s z) % 1, wrapped twice like the predictor's (the first wrap of a tiny negative value rounds to 1.0)
    for (int idx = n0 * 3 + tid; idx < n1 * 3; idx += 256) {
        const float z = philox_normal1(a.seed, to, DRAW_JUMP_X, (uint64_t)a.node_offset * 3 + idx);
        const float v = a.frac[idx] + sj * z;
        a.frac[idx] = pymod1(pymod1(v));
    }

    // atom-type logits: a = c0 a + c1 z
    for (int i = n0 + wave; i < n1; i += 4) {
        if (lane >= MI_NUM_TYPES / 4) continue;
        const int64_t idx0 = (int64_t)i * MI_NUM_TYPES + 4 * lane;
        float z[4];
        philox_normal4(a.seed, to, DRAW_JUMP_T, ((uint64_t)a.node_offset * MI_NUM_TYPES + idx0) >> 2, z);
        const f32x4 at = *reinterpret_cast<const f32x4*>(a.atom_types + idx0);
        f32x4 vout;
#pragma unroll
        for (int q = 0; q < 4; ++q) vout[q] = c0 * at[q] + c1 * z[q];
        *reinterpret_cast<f32x4*>(a.atom_types + idx0) = vout;
    }
}

// The visited levels of a chain with resampling (r, j) started at t_start: the schedule of the header, level by level.
int resample_levels(int t_start, int r, int j, std::vector<int>* levels) {
    MI_CHECK(t_start >= 0 && r >= 1 && j >= 1, MI_EINVAL, "bad resampling schedule t_start=%d r=%d j=%d (t_start >= 0, r >= 1, j >= 1)", t_start, r, j);
    std::vector<int> left((size_t)t_start + 1, 0);
    for (int64_t L = 1; L + j <= t_start; L += j) left[(size_t)L] = r - 1;
    levels->clear();
    int t = t_start;
    levels->push_back(t);
    while (t > 0) {
        --t;
        levels->push_back(t);
        if (left[(size_t)t] > 0) {
            --left[(size_t)t];
            t += j;
            levels->push_back(t);
        }
    }
    return MI_OK;
}

uint64_t resample_visit_seed(uint64_t seed, uint32_t v) {
    if (v == 0) return seed;
    const Philox4 w = philox4x32_10(0u, 0u, DRAW_VISIT, v, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (uint64_t)w.x | ((uint64_t)w.y << 32);
}

int resample_check(const mi_batch* b, int T, int t_start, int t_stop, bool has_noise, bool has_rec, const char* what) {
    if (!b->rs_on || b->rs_r <= 1) return MI_OK;
    MI_CHECK(b->cond_on, MI_EINVAL, "%s carries resampling (r = %d) and no condition: the jumps belong to a conditioned chain", what, b->rs_r);
    MI_CHECK(!has_rec, MI_EINVAL, "%s carries resampling (r = %d): a resampled chain visits levels more than once and cannot be recorded", what, b->rs_r);
    MI_CHECK(!has_noise, MI_EINVAL, "%s carries resampling (r = %d): teacher-forced noise holds one draw per level", what, b->rs_r);
    MI_CHECK(!b->lik_on, MI_EINVAL, "%s carries resampling (r = %d) AND a likelihood mask: a resampled chain has no recorded likelihood", what, b->rs_r);
    MI_CHECK(t_stop == 0, MI_EINVAL, "%s carries resampling (r = %d): the chain must run to t_stop = 0 (got %d)", what, b->rs_r, t_stop);
    MI_CHECK(b->rs_levels == T + 1, MI_EINVAL, "%s carries resampling whose jump table has %d rows, the call has T + 1 = %d", what, b->rs_levels, T + 1);
    MI_CHECK(1 + b->rs_j <= t_start, MI_EINVAL, "%s carries resampling with jump length %d: a chain started at %d has no jump-off level (1 + j <= t_start)",
             what, b->rs_j, t_start);
    return MI_OK;
}

int resample_jump(const mi_batch* b, int from_level, uint64_t seed, float* atom_types, float* frac, float* lattices, hipStream_t s) {
    MI_CHECK(b->rs_on, MI_EINVAL, "the batch handle carries no resampling");
    MI_CHECK(from_level >= 0 && from_level <= b->rs_levels - 1 - b->rs_j, MI_EINVAL, "jump %d -> %d outside the jump table (levels 0..%d)", from_level,
             from_level + b->rs_j, b->rs_levels - 1);
    if (b->B == 0 || b->N == 0) return MI_OK;
    JumpArgs a;
    a.table = b->rs_table;
    a.node_off = b->node_off;
    a.atom_types = atom_types;
    a.frac = frac;
    a.lattices = lattices;
    a.seed = seed;
    a.node_offset = b->node_offset;
    a.graph_offset = b->graph_offset;
    a.from = from_level;
    a.to = from_level + b->rs_j;
    hipLaunchKernelGGL(resample_jump_kernel, dim3(b->B), dim3(256), 0, s, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_batch_set_resampling(mi_batch* b, const float* jump_table_host, int n, int r, int j) {
    MI_NO_POOLED(b, "mi_batch_set_resampling");
    if (!jump_table_host) {
        MI_CHECK(b, MI_EINVAL, "null handle");
        b->rs_on = false;
        b->rs_r = 1;
        b->rs_j = 0;
        b->rs_levels = 0;
        return MI_OK;
    }
    // every check first, the arguments' before the handle's: a refused call leaves the handle as it was
    MI_CHECK(n >= 2, MI_EINVAL, "resampling needs a jump table of T + 1 >= 2 rows (n = %d)", n);
    MI_CHECK(r >= 1, MI_EINVAL, "resampling: r = %d visits per jump-off level, must be >= 1", r);
    MI_CHECK(j >= 1 && j < n, MI_EINVAL, "resampling: jump length j = %d, must lie in 1..%d", j, n - 1);
    for (int k = 0; k < 3 * n; ++k) MI_CHECK(std::isfinite(jump_table_host[k]), MI_EINVAL, "jump table: row %d holds a non-finite value", k / 3);
    MI_CHECK(b, MI_EINVAL, "null handle");
    b->rs_on = false;   // (a failed copy below leaves no half-written table attached)
    b->rs_levels = 0;
    if (n > b->rs_table_cap) {
        MI_TRY(dev_alloc(b, &b->rs_table, (size_t)n * 3));
        b->rs_table_cap = n;
    }
    MI_HIP(hipMemcpy(b->rs_table, jump_table_host, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
    b->rs_levels = n;
    b->rs_r = r;
    b->rs_j = j;
    b->rs_on = true;
    return MI_OK;
}

int mi_resample_jump(mi_batch* b, int from_level, uint64_t seed, float* atom_types, float* frac, float* lattices, void* stream) {
    MI_NO_POOLED(b, "mi_resample_jump");
    MI_CHECK(b && atom_types && frac && lattices, MI_EINVAL, "null argument");
    return resample_jump(b, from_level, seed, atom_types, frac, lattices, (hipStream_t)stream);
}

int64_t mi_resample_schedule(int t_start, int r, int j, int* levels_out_host, int64_t cap) {
    MI_CHECK(cap >= 0 && (levels_out_host || cap == 0), MI_EINVAL, "bad output buffer (cap = %lld)", (long long)cap);
    std::vector<int> levels;
    MI_TRY(resample_levels(t_start, r, j, &levels));
    const int64_t n = (int64_t)levels.size();
    for (int64_t k = 0; k < n && k < cap; ++k) levels_out_host[k] = levels[(size_t)k];
    return n;
}

uint64_t mi_resample_visit_seed(uint64_t seed, uint32_t v) { return resample_visit_seed(seed, v); }

}  // extern "C"
