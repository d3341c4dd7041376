// K17 -- periodic neighbour graph on gfx950: the knn branch of CSPNet.gen_edges
// (models/diffcsp/cspnet.py:243-257) = radius_graph_pbc (models/diffcsp/utils.py:335-514) +
// get_max_neighbors_mask (utils.py:517-601) + reorder_symmetric_edges (cspnet.py:159-234).
//
// Effective behaviour of the reference, restated in oracle/diffcsp_oracle.py::radius_graph_pbc / knn_edges
// and pinned by tests/golden/g5c_knn.npz:
//   * 27 periodic images (max_rep = 1), cutoff = smallest inter-plane spacing + 0.01, 1e-4 < d^2 <= cutoff^2;
//   * per centre atom, when more than `max_neighbors` candidates survive: keep d^2 < d^2_(max_neighbors) + 0.01;
//   * symmetrise: keep (j, i) with j < i (or j == i and an "earlier" image), append the flipped copies per crystal,
//     edge attribute -(x_j - x_i + image) for the kept half and its negation for the flipped half.
//
// One workgroup per crystal (crystals never interact); a wave per centre atom.  Three launches: select -> scan
// -> emit.  The emit step writes the list twice: in the reference's order (parity artefact / API output) and as
// CSR sorted by source node, which is what the message-passing kernels consume, plus the in-edge lists the
// backward pass needs.  Distances are compared, not accumulated, so contraction is off to keep the reference's
// separately rounded arithmetic.
#pragma clang fp contract(off)

#include "net.h"

namespace mi {

constexpr int KNN_NMAX = 64;  // atoms per crystal supported by the LDS-resident candidate lists

__device__ __forceinline__ void cross3(const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// ent[node][k] = (j_local << 5) | image   for the k-th kept, mask-selected neighbour of centre `node`
__global__ __launch_bounds__(256) void knn_select_kernel(const float* __restrict__ frac, const float* __restrict__ lattices,
                                                         const int* __restrict__ node_off, int max_nb, int cap, int nmax,
                                                         int* __restrict__ ent, int* __restrict__ acnt, int* __restrict__ deg,
                                                         int* __restrict__ mcount, int* __restrict__ meta) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x, n0 = node_off[b], n = node_off[b + 1] - n0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* cart = reinterpret_cast<float*>(smem);            // [nmax][3]
    float* offs = cart + 3 * nmax;                            // [27][3]
    int* degl = reinterpret_cast<int*>(offs + 81);            // [nmax]
    int* cntl = degl + nmax;                                  // [nmax]
    float* r2p = reinterpret_cast<float*>(cntl + nmax);       // [4] (1 used)
    float* dl_all = r2p + 4;                                  // [4 waves][27*nmax]
    unsigned short* ql_all = reinterpret_cast<unsigned short*>(dl_all + 4 * 27 * nmax);
    float* dl = dl_all + wave * 27 * nmax;
    unsigned short* ql = ql_all + wave * 27 * nmax;
    const float* Lm = lattices + (size_t)b * 9;

    for (int i = tid; i < n; i += 256) {
        const float* f = frac + (size_t)(n0 + i) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c)  // cart = frac @ L  (einsum "bi,bij->bj"), accumulated as a GEMM does
            cart[i * 3 + c] = __builtin_fmaf(f[2], Lm[6 + c], __builtin_fmaf(f[1], Lm[3 + c], f[0] * Lm[c]));
        degl[i] = 0;
    }
    if (tid < 27) {  // image offsets: cell^T @ unit, unit = (a, b, c) in {-1,0,1}^3, a slowest (utils.py:430-441)
        const float ua = (float)(tid / 9 - 1), ub = (float)((tid / 3) % 3 - 1), uc = (float)(tid % 3 - 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) offs[tid * 3 + c] = (Lm[c] * ua + Lm[3 + c] * ub) + Lm[6 + c] * uc;
    }
    if (tid == 0) {  // cutoff = min inter-plane spacing + 0.01 (utils.py:446-471)
        float c23[3], c31[3], c12[3];
        cross3(Lm + 3, Lm + 6, c23);
        cross3(Lm + 6, Lm, c31);
        cross3(Lm, Lm + 3, c12);
        const float vol = (Lm[0] * c23[0] + Lm[1] * c23[1]) + Lm[2] * c23[2];
        auto inv_norm = [&](const float* v) {
            const float x = v[0] / vol, y = v[1] / vol, z = v[2] / vol;
            return 1.0f / sqrtf((x * x + y * y) + z * z);
        };
        const float r = fminf(fminf(inv_norm(c23), inv_norm(c31)), inv_norm(c12)) + 0.01f;
        r2p[0] = r * r;
    }
    __syncthreads();
    const float r2 = r2p[0];
    const int nq = 27 * n;
    for (int i = wave; i < n; i += 4) {
        const float cx = cart[i * 3], cy = cart[i * 3 + 1], cz = cart[i * 3 + 2];
        int m = 0;
        for (int q0 = 0; q0 < nq; q0 += 64) {
            const int q = q0 + lane;
            bool pass = false;
            float d = 0.f;
            if (q < nq) {
                const int j = q / 27, c = q - 27 * j;
                const float dx = cx - (cart[j * 3] + offs[c * 3]), dy = cy - (cart[j * 3 + 1] + offs[c * 3 + 1]),
                            dz = cz - (cart[j * 3 + 2] + offs[c * 3 + 2]);
                d = (dx * dx + dy * dy) + dz * dz;
                pass = d <= r2 && d > 0.0001f;
            }
            const uint64_t mk = __ballot(pass);
            if (pass) {
                const int pos = m + __popcll(mk & ((1ull << lane) - 1ull));
                dl[pos] = d;
                ql[pos] = (unsigned short)q;
            }
            m += __popcll(mk);
        }
        __builtin_amdgcn_wave_barrier();
        // d^2 of the (max_nb+1)-th nearest candidate, if the list is longer than max_nb (utils.py:575-579)
        float thr = __builtin_inff();
        if (max_nb > 0 && m > max_nb) {
            float found = -__builtin_inff();
            for (int p = lane; p < m; p += 64) {
                const float v = dl[p];
                int cl = 0, cle = 0;
                for (int k = 0; k < m; ++k) {
                    const float x = dl[k];
                    cl += x < v;
                    cle += x <= v;
                }
                if (cl <= max_nb && max_nb < cle) found = v;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) found = fmaxf(found, __shfl_xor(found, o, 64));
            thr = found + 0.01f;
        }
        int cnt = 0;
        for (int p0 = 0; p0 < m; p0 += 64) {
            const int p = p0 + lane;
            bool sel = false;
            int j = 0, c = 0;
            if (p < m) {
                const int q = ql[p];
                j = q / 27;
                c = q - 27 * j;
                // reorder_symmetric_edges (cspnet.py:176-193): lower-index source, or an "earlier" image of itself
                sel = dl[p] < thr && (j < i || (j == i && c < 13));
            }
            const uint64_t mk = __ballot(sel);
            if (sel) {
                const int pos = cnt + __popcll(mk & ((1ull << lane) - 1ull));
                if (pos < cap) ent[(size_t)(n0 + i) * cap + pos] = (j << 5) | c;
                atomicAdd(&degl[j], 1);
            }
            cnt += __popcll(mk);
        }
        if (lane == 0) {
            cntl[i] = cnt;
            atomicAdd(&degl[i], cnt);
            if (cnt > cap) atomicOr(&meta[2], 1);
        }
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        acnt[n0 + i] = cntl[i];
        deg[n0 + i] = degl[i];
    }
    if (tid == 0) {
        int s = 0;
        for (int i = 0; i < n; ++i) s += cntl[i];
        mcount[b] = s;
    }
}

// eoff[b] = 2 * sum_{b' < b} mcount[b'];  rowptr = exclusive scan of deg;  meta = {E, max degree, overflow flag, STICKY capacity flag}
// meta[3] is never cleared by a build: a chain of forwards that rebuilds the list without a host round trip (knn_build nosync) leaves the verdict there, and
// mi_knn_graph_status reads it once behind the chain.  A build over capacity publishes E = 0, so that the consumers sized by capacity touch nothing.
__global__ __launch_bounds__(1024) void knn_scan_kernel(const int* __restrict__ mcount, const int* __restrict__ deg, int B, int N,
                                                         int* __restrict__ eoff, int* __restrict__ rowptr, int* __restrict__ meta, int64_t E_cap, int deg_cap) {
    __shared__ int part[1024];
    __shared__ int pmax[1024];
    const int tid = threadIdx.x;
    auto scan = [&](const int* in, int n, int mul, int* out, bool want_max) {
        const int chunk = (n + 1023) / 1024, lo = tid * chunk, hi = lo + chunk < n ? lo + chunk : n;
        int s = 0, mx = 0;
        for (int k = lo; k < hi; ++k) {
            s += in[k] * mul;
            mx = in[k] > mx ? in[k] : mx;
        }
        part[tid] = s;
        pmax[tid] = mx;
        __syncthreads();
        if (tid == 0) {
            int run = 0, m2 = 0;
            for (int k = 0; k < 1024; ++k) {
                const int v = part[k];
                part[k] = run;
                run += v;
                m2 = pmax[k] > m2 ? pmax[k] : m2;
            }
            out[n] = run;
            if (want_max) meta[1] = m2;
        }
        __syncthreads();
        int run = part[tid];
        for (int k = lo; k < hi; ++k) {
            out[k] = run;
            run += in[k] * mul;
        }
        __syncthreads();
    };
    scan(mcount, B, 2, eoff, false);
    scan(deg, N, 1, rowptr, true);
    if (tid == 0) {
        const int E = rowptr[N];
        const bool over = meta[2] != 0 || (int64_t)E > E_cap || meta[1] > deg_cap;
        meta[0] = E;
        if (over) {
            meta[2] = 1;          // (the emit kernel's test: a list over ANY capacity -- the degree's included -- is not emitted)
            meta[3] = 1;
            meta[4] = E;          // (what the host reports; the edge count the consumers see is zeroed below, after the emit kernel's own test)
            meta[5] = meta[1];
        }
        part[0] = over;
    }
    __syncthreads();
    // A list over capacity leaves NO row spans behind.  The consumers of a build without a host round trip are launched whatever the verdict, and those that walk
    // rowptr -- finalize_agg_kernel, node_chain.hip's phase A -- read one slot of mi_batch::part per 32-row block a span touches: `part` holds deg_cap / 32 + 2
    // slots, a span longer than deg_cap can touch more.  With every span empty they read nothing, and the in-edge sums of a backward pass visit nothing.
    if (part[0])
        for (int k = tid; k <= N; k += 1024) rowptr[k] = 0;
}
// behind the emit kernel of a build without a host round trip: a list over capacity was not emitted -- its consumers (sized by capacity, row count from meta[0]) get none
__global__ void knn_publish_kernel(int* __restrict__ meta, int64_t E_cap, int deg_cap) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && (meta[2] != 0 || (int64_t)meta[0] > E_cap || meta[1] > deg_cap)) meta[0] = 0;
}

__global__ __launch_bounds__(256) void knn_emit_kernel(const float* __restrict__ frac, const int* __restrict__ node_off,
                                                       const int* __restrict__ ent, const int* __restrict__ acnt,
                                                       const int* __restrict__ eoff, const int* __restrict__ rowptr, int cap, int nmax,
                                                       int64_t E_cap, int* __restrict__ r_src, int* __restrict__ r_dst,
                                                       float* __restrict__ r_vec, int* __restrict__ src, int* __restrict__ dst,
                                                       float* __restrict__ fd, int* __restrict__ edge_graph, int* __restrict__ refpos,
                                                       int* __restrict__ inedge, const int* __restrict__ meta) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (meta[2] != 0 || (int64_t)meta[0] > E_cap) return;  // capacity exceeded: the host raises after the launch
    const int b = blockIdx.x, n0 = node_off[b], n = node_off[b + 1] - n0, tid = threadIdx.x;
    int* aoff = reinterpret_cast<int*>(smem);  // [nmax + 1]
    int* el = aoff + nmax + 1;                 // [n * cap] entries of the crystal: (i << 16) | (j << 5) | image
    if (tid == 0) {
        int s = 0;
        for (int i = 0; i < n; ++i) {
            aoff[i] = s;
            s += acnt[n0 + i];
        }
        aoff[n] = s;
    }
    __syncthreads();
    const int M = aoff[n], e0 = eoff[b];
    for (int i = 0; i < n; ++i)
        for (int k = tid; k < aoff[i + 1] - aoff[i]; k += 256) el[aoff[i] + k] = (i << 16) | ent[(size_t)(n0 + i) * cap + k];
    __syncthreads();
    // reference order (cspnet.py:195-234): the kept half in (i, j, image) order, then the flipped half
    for (int t = tid; t < M; t += 256) {
        const int w = el[t], i = w >> 16, j = (w >> 5) & 0x7ff, c = w & 31;
        const float im[3] = {(float)(c / 9 - 1), (float)((c / 3) % 3 - 1), (float)(c % 3 - 1)};
        r_src[e0 + t] = n0 + j;
        r_dst[e0 + t] = n0 + i;
        r_src[e0 + M + t] = n0 + i;
        r_dst[e0 + M + t] = n0 + j;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = (frac[(size_t)(n0 + j) * 3 + a] - frac[(size_t)(n0 + i) * 3 + a]) + im[a];  // cspnet.py:249
            r_vec[(size_t)(e0 + t) * 3 + a] = -v;
            r_vec[(size_t)(e0 + M + t) * 3 + a] = v;
        }
    }
    __syncthreads();
    // CSR by source node: row v = [kept-half edges with source v] ++ [flipped-half edges with source v], each in list order
    for (int v = tid; v < n; v += 256) {
        int cur = rowptr[n0 + v];
        for (int t = 0; t < M; ++t) {
            const int w = el[t];
            if (((w >> 5) & 0x7ff) == v) {
                refpos[e0 + t] = cur;
                ++cur;
            }
        }
        for (int t = aoff[v]; t < aoff[v + 1]; ++t) {
            refpos[e0 + M + t] = cur;
            ++cur;
        }
    }
    __threadfence_block();
    __syncthreads();
    for (int r = tid; r < 2 * M; r += 256) {
        const int p = refpos[e0 + r];
        src[p] = r_src[e0 + r];
        dst[p] = r_dst[e0 + r];
        edge_graph[p] = b;
#pragma unroll
        for (int a = 0; a < 3; ++a) fd[(size_t)p * 3 + a] = r_vec[(size_t)(e0 + r) * 3 + a];
    }
    // in-edges of v = the flipped partners of its out-edges (the list is symmetric), same order as row v
    for (int v = tid; v < n; v += 256) {
        int cur = rowptr[n0 + v];
        for (int t = 0; t < M; ++t)
            if (((el[t] >> 5) & 0x7ff) == v) inedge[cur++] = refpos[e0 + M + t];
        for (int t = aoff[v]; t < aoff[v + 1]; ++t) inedge[cur++] = refpos[e0 + t];
    }
}

// K18 -- geometric validity pre-filter of sampled structures, straight off the sampler's final state: the cell test of
// pipeline/filters/opt_filter.py:53-55 (max cell edge < 25 A is applied by the caller on `max_len`) and the quantities the
// external structure_validity check thresholds (shortest interatomic distance incl. periodic images, cell volume).
// out[b] = {longest cell edge, shortest distance, |det L|, number of atoms}.  One workgroup per crystal; pairs x 27 images.
__global__ __launch_bounds__(256) void structure_check_kernel(const float* __restrict__ frac, const float* __restrict__ lattices,
                                                              const int* __restrict__ node_off, float* __restrict__ out) {
    __shared__ float red[256];
    __shared__ float offs[81];
    const int b = blockIdx.x, n0 = node_off[b], n = node_off[b + 1] - n0, tid = threadIdx.x;
    const float* Lm = lattices + (size_t)b * 9;
    if (tid < 27) {
        const float ua = (float)(tid / 9 - 1), ub = (float)((tid / 3) % 3 - 1), uc = (float)(tid % 3 - 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) offs[tid * 3 + c] = (Lm[c] * ua + Lm[3 + c] * ub) + Lm[6 + c] * uc;
    }
    __syncthreads();
    float best = __builtin_inff();
    const int64_t total = (int64_t)n * n * 27;
    for (int64_t w = tid; w < total; w += 256) {
        const int c = (int)(w % 27), j = (int)((w / 27) % n), i = (int)(w / (27 * (int64_t)n));
        if (j < i || (j == i && c == 13)) continue;  // unordered pairs; an atom and its own home image is not a pair
        float d[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) d[a] = frac[(size_t)(n0 + j) * 3 + a] - frac[(size_t)(n0 + i) * 3 + a];
        float s = 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float x = ((d[0] * Lm[a] + d[1] * Lm[3 + a]) + d[2] * Lm[6 + a]) + offs[c * 3 + a];
            s += x * x;
        }
        best = fminf(best, s);
    }
    red[tid] = best;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fminf(red[tid], red[tid + o]);
        __syncthreads();
    }
    if (tid == 0) {
        float len = 0.f;
#pragma unroll
        for (int r = 0; r < 3; ++r) len = fmaxf(len, sqrtf((Lm[r * 3] * Lm[r * 3] + Lm[r * 3 + 1] * Lm[r * 3 + 1]) + Lm[r * 3 + 2] * Lm[r * 3 + 2]));
        float c23[3];
        cross3(Lm + 3, Lm + 6, c23);
        out[b * 4 + 0] = len;
        out[b * 4 + 1] = sqrtf(red[0]);
        out[b * 4 + 2] = fabsf((Lm[0] * c23[0] + Lm[1] * c23[1]) + Lm[2] * c23[2]);
        out[b * 4 + 3] = (float)n;
    }
}

static size_t select_lds(int nmax) { return (size_t)(3 * nmax + 81 + 2 * nmax + 4) * 4 + (size_t)4 * 27 * nmax * (4 + 2); }
static size_t emit_lds(int nmax, int cap) { return (size_t)(nmax + 1 + (size_t)nmax * cap) * 4; }

int knn_alloc(mi_batch* b, int max_neighbors, int cap_per_node) {
    int nmax = 1;
    for (int n : b->num_atoms_h) nmax = std::max(nmax, n);
    MI_CHECK(nmax <= KNN_NMAX, MI_EINVAL, "knn graph: %d atoms in one crystal exceeds the supported %d", nmax, KNN_NMAX);
    MI_CHECK(max_neighbors >= 0 && cap_per_node >= 1 && cap_per_node <= 27 * KNN_NMAX, MI_EINVAL, "knn graph: bad max_neighbors / capacity");
    MI_CHECK(emit_lds(nmax, cap_per_node) <= 64 * 1024, MI_EINVAL, "knn graph: capacity %d per atom x %d atoms exceeds the emit kernel's LDS budget",
             cap_per_node, nmax);
    b->knn = 1;
    b->max_neighbors = max_neighbors;
    b->cap_per_node = cap_per_node;
    b->nmax = nmax;
    b->deg_cap = 2 * cap_per_node;
    b->E_cap = (int64_t)b->N * 2 * cap_per_node;
    int rc = MI_OK;
    const size_t N = b->N, B = b->B, EC = (size_t)b->E_cap;
#define A_(p, n) if (rc == MI_OK) rc = dev_alloc(b, &b->p, (n))
    A_(kn_ent, N * cap_per_node);
    A_(kn_acnt, N);
    A_(kn_deg, N);
    A_(kn_mcount, B);
    A_(kn_eoff, B + 1);
    A_(kn_meta, 8);
    A_(kn_refpos, EC);
    A_(r_src, EC);
    A_(r_dst, EC);
    A_(r_vec, EC * 3);
    A_(fd, EC * 3);
    A_(inedge, EC);
#undef A_
    if (rc == MI_OK && b->kn_meta && hipMemset(b->kn_meta, 0, 8 * sizeof(int)) != hipSuccess) rc = MI_EHIP;   // (the sticky verdict meta[3..5] starts clean: a build clears meta[0..2] only)
    return rc;
}

// Rebuild the edge list of a knn batch from the current coordinates.  One host synchronisation (the edge count
// sizes every later launch).
int knn_build(mi_batch* b, const float* frac, const float* lattices, hipStream_t s, bool nosync) {
    MI_CHECK(b->knn, MI_ESTATE, "batch was not created with the knn edge style");
    b->E = 0;
    b->e_dev = nullptr;
    if (b->N == 0 || b->B == 0) return MI_OK;
    MI_HIP(hipMemsetAsync(b->kn_meta, 0, 3 * sizeof(int), s));   // (meta[3..5]: the sticky capacity verdict of a chain of builds, cleared by mi_knn_graph_status)
    hipLaunchKernelGGL(knn_select_kernel, dim3(b->B), dim3(256), select_lds(b->nmax), s, frac, lattices, b->node_off, b->max_neighbors,
                       b->cap_per_node, b->nmax, b->kn_ent, b->kn_acnt, b->kn_deg, b->kn_mcount, b->kn_meta);
    hipLaunchKernelGGL(knn_scan_kernel, dim3(1), dim3(1024), 0, s, b->kn_mcount, b->kn_deg, b->B, b->N, b->kn_eoff, b->rowptr, b->kn_meta, b->E_cap, b->deg_cap);
    hipLaunchKernelGGL(knn_emit_kernel, dim3(b->B), dim3(256), emit_lds(b->nmax, b->cap_per_node), s, frac, b->node_off, b->kn_ent, b->kn_acnt,
                       b->kn_eoff, b->rowptr, b->cap_per_node, b->nmax, b->E_cap, b->r_src, b->r_dst, b->r_vec, b->src, b->dst, b->fd,
                       b->edge_graph, b->kn_refpos, b->inedge, b->kn_meta);
    MI_KERNEL_CHECK();
    ++b->graph_epoch;   // (tables derived from the edge list -- edge_stage.hip's per-tile tables -- are rebuilt at their next use)
    if (nosync && (b->e_hint > 0 || g_knn_nosync == 2)) {   // (the very first build of a handle synchronises once: the host learns the list's size, which picks the kernel forms from then on; 2 = not even that one, tests)
        // No host round trip: the consumers are launched for the CAPACITY and take the row count from meta[0] on the device (PlanesEpilogue::m_dev, the
        // Fourier operand's e_dev); tiles past the count exit at once.  A list over capacity sets the sticky flag meta[3] and publishes zero edges; the
        // caller of the chain asks mi_knn_graph_status once behind it (the error is the same MI_ECAPACITY, raised later instead of never).
        hipLaunchKernelGGL(knn_publish_kernel, dim3(1), dim3(64), 0, s, b->kn_meta, b->E_cap, b->deg_cap);
        MI_KERNEL_CHECK();
        b->E = b->E_cap;
        b->e_dev = b->kn_meta;
        return MI_OK;
    }
    int meta[4];
    MI_HIP(hipMemcpyAsync(meta, b->kn_meta, sizeof(meta), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    if (meta[3] != 0) MI_HIP(hipMemsetAsync(b->kn_meta + 3, 0, 3 * sizeof(int), s));   // (this build reports for itself, right here)
    MI_CHECK(meta[2] == 0 && meta[0] <= b->E_cap && meta[1] <= b->deg_cap, MI_ECAPACITY,
             "knn graph exceeds its capacity (edges %d of %lld, max degree %d of %d): raise edge_cap_per_node", meta[0], (long long)b->E_cap,
             meta[1], b->deg_cap);
    b->E = meta[0];
    b->e_hint = std::max<int64_t>(meta[0], 1);
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_knn_graph(mi_batch* b, const float* frac, const float* lattices, void* stream, int64_t* num_edges) {
    MI_CHECK(b && frac && lattices, MI_EINVAL, "null argument");
    MI_TRY(knn_build(b, frac, lattices, (hipStream_t)stream));
    if (num_edges) *num_edges = b->E;
    return MI_OK;
}

int mi_knn_graph_status(mi_batch* b, void* stream) {
    MI_CHECK(b && b->knn, MI_ESTATE, "batch was not created with the knn edge style");
    if (b->N == 0 || b->B == 0) return MI_OK;
    hipStream_t s = (hipStream_t)stream;
    int meta[8];
    MI_HIP(hipMemcpyAsync(meta, b->kn_meta, sizeof(meta), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    if (meta[3] != 0) {
        MI_HIP(hipMemsetAsync(b->kn_meta + 3, 0, 3 * sizeof(int), s));
        b->E = 0;             // (nothing on the handle describes a list any more: mi_batch_num_edges and mi_knn_graph_read report none)
        b->e_dev = nullptr;
        mi::set_error("a knn graph built inside the chain exceeded its capacity (edges %d of %lld, max degree %d of %d): the chain's results are invalid; raise edge_cap_per_node",
                      meta[4], (long long)b->E_cap, meta[5], b->deg_cap);
        return MI_ECAPACITY;
    }
    // The host has now seen the count of the chain's last list: the handle describes that list, not its capacity (a build without a host round trip left
    // E = E_cap and e_dev set; mi_batch_num_edges and mi_knn_graph_read go by E).  Every forward of a knn handle rebuilds the list and sets both again.
    b->E = std::min<int64_t>(meta[0], b->E_cap);
    b->e_dev = nullptr;
    b->e_hint = std::max<int64_t>(meta[0], 1);   // (the size of the chain's last list: the form hint of the next chain's launches)
    return MI_OK;
}

int mi_structure_check_offsets(const int* node_off, int B, const float* frac, const float* lattices, float* out, void* stream) {
    MI_CHECK(node_off && frac && lattices && out && B >= 0, MI_EINVAL, "bad argument");
    if (B == 0) return MI_OK;
    hipLaunchKernelGGL(structure_check_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, frac, lattices, node_off, out);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int mi_structure_check(const mi_batch* b, const float* frac, const float* lattices, float* out, void* stream) {
    MI_POOL_STREAM(b, stream, "mi_structure_check");
    MI_CHECK(b && frac && lattices && out, MI_EINVAL, "null argument");
    if (b->B == 0) return MI_OK;
    hipLaunchKernelGGL(structure_check_kernel, dim3(b->B), dim3(256), 0, (hipStream_t)stream, frac, lattices, b->node_off, out);
    MI_KERNEL_CHECK();
    return MI_OK;
}

int mi_knn_graph_read(const mi_batch* b, int* edges, float* edge_vec, int order, void* stream) {
    MI_CHECK(b && b->knn, MI_ESTATE, "batch was not created with the knn edge style");
    MI_CHECK(order == 0 || order == 1, MI_EINVAL, "order must be MI_EDGE_ORDER_REFERENCE (0) or MI_EDGE_ORDER_CSR (1)");
    const size_t E = (size_t)b->E;
    if (E == 0) return MI_OK;
    hipStream_t s = (hipStream_t)stream;
    if (edges) {
        MI_HIP(hipMemcpyAsync(edges, order == 0 ? b->r_src : b->src, E * sizeof(int), hipMemcpyDeviceToDevice, s));
        MI_HIP(hipMemcpyAsync(edges + E, order == 0 ? b->r_dst : b->dst, E * sizeof(int), hipMemcpyDeviceToDevice, s));
    }
    if (edge_vec) MI_HIP(hipMemcpyAsync(edge_vec, order == 0 ? b->r_vec : b->fd, E * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return MI_OK;
}

}  // extern "C"
