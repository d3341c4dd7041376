// Symmetry-constrained sampling (include/matinvent_hip_symc.h): a batch handle's symmetry constraint and the one kernel that
// projects a state of the reverse chain onto it.  One launch, no atomics, no scratch, no matrix pipe, nothing waits for the host:
//   symmetry_project_kernel   one 256-thread workgroup per crystal.  A thread per atom reads its REPRESENTATIVE's coordinates and forms its
//                             own from them; a thread per distinct rotation part forms its congruence of the metric.  Behind one barrier
//                             -- every read of the crystal's coordinates and cell precedes every write -- the nine sums go through one
//                             fixed tree over LDS, the coordinates are stored, thread 0 factors the mean metric, and the type rows of the
//                             representatives are copied to their orbits in a strided loop over (atom, float4 column).
// csrc/sym_constraint.h holds every formula, host and device.

#include <cmath>
#include <vector>

#include "../../include/matinvent_hip_symc.h"
#include "net.h"
#include "sym_constraint.h"

namespace mi {

static_assert(SYMC_MAX_ATOMS == MI_SYMC_MAX_ATOMS && SYMC_MAX_OPS == MI_SYMC_MAX_OPS, "constants");
static_assert(SYMC_MAX_ATOMS <= SYMC_THREADS && SYMC_MAX_OPS <= SYMC_THREADS, "a thread per atom; a thread per rotation part");
static_assert(SYMC_QUADS * 4 == MI_NUM_TYPES, "a type row is 25 float4 columns");

struct SymcArgs {
    const int *K, *roff, *rot, *rep, *node_off;   // [B], [B + 1], [roff[B]][9], [N], [B + 1]
    const double *Q, *d;                          // [N][9], [N][3]
    int* fail;                                    // [B]
    float *atom_types, *frac, *lattices;          // the state, projected in place
};

__global__ __launch_bounds__(SYMC_THREADS) void symmetry_project_kernel(SymcArgs a) {
    __shared__ double s_red[9][SYMC_THREADS];
    __shared__ int s_rep[SYMC_MAX_ATOMS];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (a.K[b] <= 1) return;   // (uniform) the identity alone: every bit stays
    const int n0 = a.node_off[b], n = a.node_off[b + 1] - n0;   // (n <= 256: mi_batch_set_symmetry checked)
    const int r0 = a.roff[b], R = a.roff[b + 1] - r0;
    // ---- the reads: the representative's coordinates, the cell
    float x[3] = {0.f, 0.f, 0.f};
    if (tid < n) {
        const int r = a.rep[n0 + tid];
        s_rep[tid] = r;
        float xr[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) xr[c] = a.frac[(size_t)(n0 + r) * 3 + c];
        symc_coord(xr, a.Q + (size_t)(n0 + tid) * 9, a.d + (size_t)(n0 + tid) * 3, x);
    }
    {
        float lat32[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) lat32[e] = a.lattices[(size_t)b * 9 + e];
        double G[9], Gk[9];
        symc_metric(lat32, G);
        symc_slot(a.rot + (size_t)r0 * 9, R, tid, G, Gk);
#pragma unroll
        for (int e = 0; e < 9; ++e) s_red[e][tid] = Gk[e];
    }
    __syncthreads();
    // ---- the fixed tree over the 256 slots
    for (int s = SYMC_THREADS / 2; s >= 1; s >>= 1) {   // (uniform)
        if (tid < s) {
#pragma unroll
            for (int e = 0; e < 9; ++e) s_red[e][tid] = refine_tree_add(s_red[e][tid], s_red[e][tid + s]);
        }
        __syncthreads();
    }
    // ---- the writes
    if (tid < n) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.frac[(size_t)(n0 + tid) * 3 + c] = x[c];
    }
    if (tid == 0) {
        double Gsum[9];
        float cell[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) Gsum[e] = s_red[e][0];
        if (symc_cell(Gsum, R, cell)) {
#pragma unroll
            for (int e = 0; e < 9; ++e) a.lattices[(size_t)b * 9 + e] = cell[e];
        } else {
            a.fail[b] = a.fail[b] + 1;   // this crystal's own workgroup is the counter's only writer
        }
    }
    // the type rows: a representative's row is read and never written, every other row is written and never read
    for (int item = tid; item < n * SYMC_QUADS; item += SYMC_THREADS) {
        const int j = item / SYMC_QUADS, q = item - j * SYMC_QUADS, r = s_rep[j];
        if (r == j) continue;
        const f32x4 v = *reinterpret_cast<const f32x4*>(a.atom_types + (size_t)(n0 + r) * MI_NUM_TYPES + 4 * q);
        *reinterpret_cast<f32x4*>(a.atom_types + (size_t)(n0 + j) * MI_NUM_TYPES + 4 * q) = v;
    }
}

int symmetry_check(const mi_batch* b, bool has_noise, bool has_rec, const char* what) {
    if (!b->symc_on) return MI_OK;
    MI_CHECK(!has_rec, MI_EINVAL, "%s carries a symmetry constraint AND the call records: a projected state has no likelihood under the recorded proposal", what);
    MI_CHECK(!has_noise, MI_EINVAL, "%s carries a symmetry constraint AND the call is given teacher-forced noise", what);
    MI_CHECK(!b->keep_lattice && !b->keep_coords, MI_EINVAL, "%s carries a symmetry constraint AND CSP mode (keep_lattice / keep_coords)", what);
    MI_CHECK(!(b->rs_on && b->rs_r > 1), MI_EINVAL, "%s carries a symmetry constraint AND resampling jumps (r = %d)", what, b->rs_r);
    MI_CHECK(!b->gd_on, MI_EINVAL, "%s carries a symmetry constraint AND guidance", what);
    MI_CHECK(!b->cond_on || (!b->cond_has_x && !b->cond_has_l), MI_EINVAL,
             "%s carries a symmetry constraint AND a condition that knows a coordinate or a lattice: only a condition on atom types goes with it", what);
    return MI_OK;
}

int symmetry_impose(const mi_batch* b, float* atom_types, float* frac, float* lattices, hipStream_t s) {
    MI_CHECK(b->symc_on, MI_EINVAL, "the batch handle carries no symmetry constraint");
    MI_CHECK(((uintptr_t)atom_types & 15) == 0, MI_EINVAL, "the type rows must be 16-byte aligned");
    if (!b->symc_any || b->B == 0 || b->N == 0) return MI_OK;
    SymcArgs a;
    a.K = b->symc_K;
    a.roff = b->symc_roff;
    a.rot = b->symc_rot;
    a.rep = b->symc_rep;
    a.node_off = b->node_off;
    a.Q = b->symc_Q;
    a.d = b->symc_d;
    a.fail = b->symc_fail;
    a.atom_types = atom_types;
    a.frac = frac;
    a.lattices = lattices;
    hipLaunchKernelGGL(symmetry_project_kernel, dim3(b->B), dim3(SYMC_THREADS), 0, s, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // namespace mi

using namespace mi;

namespace {
template <typename T>
int upload(mi_batch* b, T** dev, const T* host, size_t n) {
    if (!*dev) MI_TRY(dev_alloc(b, dev, n));
    if (n) MI_HIP(hipMemcpy(*dev, host, n * sizeof(T), hipMemcpyHostToDevice));
    return MI_OK;
}

bool same_rot(const int* p, const int* q) {
    for (int e = 0; e < 9; ++e)
        if (p[e] != q[e]) return false;
    return true;
}
}  // namespace

extern "C" {

int mi_batch_set_symmetry(mi_batch* b, const mi_symmetry_constraint* c) {
    MI_NO_POOLED(b, "mi_batch_set_symmetry");
    MI_CHECK(b, MI_EINVAL, "null handle");
    if (!c) {
        b->symc_on = b->symc_any = false;
        return MI_OK;
    }
    // every check first: a refused call leaves the handle as it was
    MI_CHECK(c->op_off_host && c->rot_host && c->distinct_off_host && c->distinct_host, MI_EINVAL, "symmetry constraint: null operation array");
    const int N = b->N, B = b->B;
    MI_CHECK(N == 0 || (c->rep_host && c->Q_host && c->d_host), MI_EINVAL, "symmetry constraint: null atom array");
    MI_CHECK(c->op_off_host[0] == 0 && c->distinct_off_host[0] == 0, MI_EINVAL, "symmetry constraint: the offsets must start at 0");
    std::vector<int> K((size_t)B), rot;
    bool any = false;
    for (int g = 0; g < B; ++g) {
        const int k0 = c->op_off_host[g], Kg = c->op_off_host[g + 1] - k0;
        MI_CHECK(Kg >= 1 && Kg <= MI_SYMC_MAX_OPS, MI_EINVAL, "symmetry constraint: crystal %d has %d operations (1..%d)", g, Kg, MI_SYMC_MAX_OPS);
        const int n0 = b->node_off_h[(size_t)g], n = b->node_off_h[(size_t)g + 1] - n0;
        MI_CHECK(Kg == 1 || n <= MI_SYMC_MAX_ATOMS, MI_EINVAL, "symmetry constraint: crystal %d has %d atoms (at most %d)", g, n, MI_SYMC_MAX_ATOMS);
        const int* W = c->rot_host + (size_t)k0 * 9;
        for (int k = 0; k < Kg; ++k) MI_CHECK(symc_unimodular(W + 9 * k), MI_EINVAL, "symmetry constraint: crystal %d, operation %d: det W is not +-1", g, k);
        const int d0 = c->distinct_off_host[g], R = c->distinct_off_host[g + 1] - d0;
        MI_CHECK(R >= 1 && R <= Kg, MI_EINVAL, "symmetry constraint: crystal %d lists %d distinct rotation parts of %d operations", g, R, Kg);
        const int* D = c->distinct_host + d0;
        for (int i = 0; i < R; ++i) {
            MI_CHECK(D[i] >= 0 && D[i] < Kg, MI_EINVAL, "symmetry constraint: crystal %d: distinct entry %d = %d leaves its %d operations", g, i, D[i], Kg);
            for (int j = 0; j < i; ++j)
                MI_CHECK(!same_rot(W + 9 * D[i], W + 9 * D[j]), MI_EINVAL, "symmetry constraint: crystal %d: distinct entries %d and %d hold the same rotation part", g, j, i);
        }
        for (int k = 0; k < Kg; ++k) {
            bool found = false;
            for (int i = 0; i < R && !found; ++i) found = same_rot(W + 9 * k, W + 9 * D[i]);
            MI_CHECK(found, MI_EINVAL, "symmetry constraint: crystal %d: the rotation part of operation %d is not in the distinct list", g, k);
        }
        for (int i = 0; i < n; ++i) {
            const int r = c->rep_host[n0 + i];
            MI_CHECK(r >= 0 && r < n, MI_EINVAL, "symmetry constraint: crystal %d, atom %d: representative %d outside the crystal's %d atoms", g, i, r, n);
            MI_CHECK(c->rep_host[n0 + r] == r, MI_EINVAL, "symmetry constraint: crystal %d, atom %d: representative %d is not its own representative", g, i, r);
            for (int e = 0; e < 9; ++e) MI_CHECK(std::isfinite(c->Q_host[(size_t)(n0 + i) * 9 + e]), MI_EINVAL, "symmetry constraint: crystal %d, atom %d: non-finite Q", g, i);
            for (int e = 0; e < 3; ++e) MI_CHECK(std::isfinite(c->d_host[(size_t)(n0 + i) * 3 + e]), MI_EINVAL, "symmetry constraint: crystal %d, atom %d: non-finite d", g, i);
        }
        K[(size_t)g] = Kg;
        any = any || Kg > 1;
        for (int i = 0; i < R; ++i) rot.insert(rot.end(), W + 9 * D[i], W + 9 * D[i] + 9);
    }

    b->symc_on = b->symc_any = false;   // (a failed copy below leaves no half-written constraint attached)
    const int nrot = (int)(rot.size() / 9);
    if (nrot > b->symc_rot_cap) {
        if (b->symc_rot) dev_release(b, b->symc_rot);
        b->symc_rot = nullptr, b->symc_rot_cap = 0;
        MI_TRY(dev_alloc(b, &b->symc_rot, rot.size()));
        b->symc_rot_cap = nrot;
    }
    if (nrot) MI_HIP(hipMemcpy(b->symc_rot, rot.data(), rot.size() * sizeof(int), hipMemcpyHostToDevice));
    MI_TRY(upload(b, &b->symc_K, (const int*)K.data(), (size_t)B));
    MI_TRY(upload(b, &b->symc_roff, c->distinct_off_host, (size_t)B + 1));
    MI_TRY(upload(b, &b->symc_rep, c->rep_host, (size_t)N));
    MI_TRY(upload(b, &b->symc_Q, c->Q_host, (size_t)N * 9));
    MI_TRY(upload(b, &b->symc_d, c->d_host, (size_t)N * 3));
    if (!b->symc_fail) MI_TRY(dev_alloc(b, &b->symc_fail, (size_t)B));
    MI_HIP(hipMemset(b->symc_fail, 0, (size_t)std::max(B, 1) * sizeof(int)));
    b->symc_any = any;
    b->symc_on = true;
    return MI_OK;
}

int mi_symmetry_apply(mi_batch* b, float* atom_types, float* frac, float* lattices, void* stream) {
    MI_NO_POOLED(b, "mi_symmetry_apply");
    MI_CHECK(b && atom_types && frac && lattices, MI_EINVAL, "null argument");
    return symmetry_impose(b, atom_types, frac, lattices, (hipStream_t)stream);
}

int mi_symmetry_failures(mi_batch* b, int* out_host) {
    MI_NO_POOLED(b, "mi_symmetry_failures");
    MI_CHECK(b && out_host, MI_EINVAL, "null argument");
    MI_CHECK(b->symc_on, MI_EINVAL, "the batch handle carries no symmetry constraint");
    if (b->B == 0) return MI_OK;
    MI_HIP(hipMemcpy(out_host, b->symc_fail, (size_t)b->B * sizeof(int), hipMemcpyDeviceToHost));
    MI_HIP(hipMemset(b->symc_fail, 0, (size_t)b->B * sizeof(int)));
    return MI_OK;
}

}  // extern "C"
