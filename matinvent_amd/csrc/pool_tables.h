// The index tables of a fully connected batch handle, decoded per element from three prefix arrays (pool.hip's kernels).
// Host and device: scripts/pool_tables_host_check.cpp compiles these functions for the host and compares every value with the loops of
// batch_create_impl (cspnet.hip), which stay the definition.  Integer arithmetic decides every value; the one square root is a first
// guess that two integer loops correct.
//
//   node_off [B + 1]  sum of n          node v of crystal g: local index i = v - node_off[g]
//   edge_off [B + 1]  sum of n^2        edge e of crystal g: row-major (i, j), e = edge_off[g] + i n + j (self loops included)
//   pair_off [B + 1]  sum of n (n-1)/2  pair p of crystal g: i ascending, then j = i + 1 .. n - 1
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MI_PT_HD __host__ __device__
#else
#define MI_PT_HD
#endif

namespace mi {

struct PoolTables {
    const int *node_off, *edge_off, *pair_off;   // [B + 1] each
    int B;
    int *num_atoms, *node2graph, *rowptr, *e_diag;                 // [B], [N], [N + 1], [N]
    int *src, *dst, *edge_graph;                                   // [E]
    int *pair_i, *pair_j, *pair_e1, *pair_e2, *pair_graph;         // [Np]
};

// the crystal g with off[g] <= x < off[g + 1] (crystals without elements are stepped over); 0 <= x < off[B]
MI_PT_HD inline int pt_find(const int* off, int B, int64_t x) {
    int lo = 0, hi = B;   // the answer lies in [lo, hi)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if ((int64_t)off[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// pairs in front of row i of a crystal of n atoms: sum_{k < i} (n - 1 - k)
MI_PT_HD inline int64_t pt_row_start(int64_t i, int64_t n) { return i * (2 * n - i - 1) / 2; }

// the row i of pair q (0 <= q < n (n - 1) / 2) of a crystal of n >= 2 atoms: the largest i with pt_row_start(i, n) <= q
MI_PT_HD inline int pt_pair_row(int64_t q, int n) {
    const double t = 2.0 * n - 1.0;
    double d = t * t - 8.0 * (double)q;
    if (d < 0.0) d = 0.0;
    int64_t i = (int64_t)((t - sqrt(d)) * 0.5);
    if (i < 0) i = 0;
    if (i > n - 2) i = n - 2;
    while (i > 0 && pt_row_start(i, n) > q) --i;
    while (i < n - 2 && pt_row_start(i + 1, n) <= q) ++i;
    return (int)i;
}

// crystal g (0 <= g < B)
MI_PT_HD inline void pt_crystal(const PoolTables& t, int g) { t.num_atoms[g] = t.node_off[g + 1] - t.node_off[g]; }

// node v (0 <= v < N); v == N writes the closing entry of rowptr
MI_PT_HD inline void pt_node(const PoolTables& t, int v) {
    const int N = t.node_off[t.B];
    if (v == N) {
        t.rowptr[N] = t.edge_off[t.B];
        return;
    }
    const int g = pt_find(t.node_off, t.B, v);
    const int o = t.node_off[g], n = t.node_off[g + 1] - o, i = v - o;
    const int rp = t.edge_off[g] + i * n;
    t.node2graph[v] = g;
    t.rowptr[v] = rp;
    t.e_diag[v] = rp + i;
}

// edge e (0 <= e < E)
MI_PT_HD inline void pt_edge(const PoolTables& t, int64_t e) {
    const int g = pt_find(t.edge_off, t.B, e);
    const int o = t.node_off[g], n = t.node_off[g + 1] - o;
    const int r = (int)(e - t.edge_off[g]);
    t.src[e] = o + r / n;
    t.dst[e] = o + r % n;
    t.edge_graph[e] = g;
}

// pair p (0 <= p < Np)
MI_PT_HD inline void pt_pair(const PoolTables& t, int64_t p) {
    const int g = pt_find(t.pair_off, t.B, p);
    const int o = t.node_off[g], n = t.node_off[g + 1] - o, e0 = t.edge_off[g];
    const int64_t q = p - t.pair_off[g];
    const int i = pt_pair_row(q, n);
    const int j = i + 1 + (int)(q - pt_row_start(i, n));
    t.pair_i[p] = o + i;
    t.pair_j[p] = o + j;
    t.pair_e1[p] = e0 + i * n + j;
    t.pair_e2[p] = e0 + j * n + i;
    t.pair_graph[p] = g;
}

// the block-sum slots the edge -> node reduction needs: the largest number of 32-edge blocks one node's row of edges touches
MI_PT_HD inline int pt_node_slots(int rowptr, int n) { return ((rowptr + n - 1) >> 5) - (rowptr >> 5) + 1; }

}  // namespace mi
