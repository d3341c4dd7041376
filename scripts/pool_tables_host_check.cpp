// The index-table decode of a pooled batch handle (matinvent_amd/csrc/pool_tables.h: what pool.hip's kernels run per node, edge and pair)
// run on the host and compared, value for value, with the literal loops of batch_create_impl (cspnet.hip), which stay the definition.
// Every array is allocated at exactly its size, so that the host sanitizers see any index past an end:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/pool_tables_host_check.cpp -o pool_tables_host_check
//   ./pool_tables_host_check
//
// Cases: every single crystal of 1 .. 200 atoms; [1, 7, 20, 3, 13]; 300 crystals with counts cycling 1 .. 5; and two lists with empty
// crystals.  Exit status 0: every table of every case is equal; 1: a mismatch (printed).
#include <algorithm>
#include <cstdio>
#include <memory>
#include <vector>

#include "../matinvent_amd/csrc/pool_tables.h"

using namespace mi;

static int check(const std::vector<int>& na, const char* what) {
    const int B = (int)na.size();
    // ---- the loops of batch_create_impl ----
    std::vector<int> node_off(B + 1, 0);
    for (int g = 0; g < B; ++g) node_off[g + 1] = node_off[g] + na[g];
    const int N = node_off[B];
    std::vector<int> n2g(N), src, dst, egraph, rowptr(N + 1, 0), ediag(N), pr_i, pr_j, pr_e1, pr_e2, pr_g, pr_off(B + 1, 0);
    size_t e = 0;
    int nslots = 1, nmax = 0;
    for (int g = 0; g < B; ++g) {
        const int n = na[g], o = node_off[g];
        for (int i = 0; i < n; ++i) {
            n2g[o + i] = g;
            rowptr[o + i] = (int)e;
            for (int j = 0; j < n; ++j) {
                src.push_back(o + i);
                dst.push_back(o + j);
                egraph.push_back(g);
                ++e;
            }
            nslots = std::max(nslots, (int)((e - 1) >> 5) - (rowptr[o + i] >> 5) + 1);
        }
        pr_off[g] = (int)pr_i.size();
        nmax = std::max(nmax, n);
        for (int i = 0; i < n; ++i) {
            ediag[o + i] = rowptr[o + i] + i;
            for (int j = i + 1; j < n; ++j) {
                pr_i.push_back(o + i);
                pr_j.push_back(o + j);
                pr_e1.push_back(rowptr[o + i] + j);
                pr_e2.push_back(rowptr[o + j] + i);
                pr_g.push_back(g);
            }
        }
    }
    pr_off[B] = (int)pr_i.size();
    rowptr[N] = (int)e;
    const int64_t E = (int64_t)e, Np = (int64_t)pr_i.size();
    // ---- the pooled route: three prefix sums and nslots on the host, everything else decoded per element ----
    std::unique_ptr<int[]> noff(new int[B + 1]), eoff(new int[B + 1]), poff(new int[B + 1]);
    noff[0] = eoff[0] = poff[0] = 0;
    int nslots2 = 1;
    for (int g = 0; g < B; ++g) {
        const int n = na[g];
        noff[g + 1] = noff[g] + n;
        eoff[g + 1] = eoff[g] + n * n;
        poff[g + 1] = poff[g] + n * (n - 1) / 2;
        for (int i = 0; i < n; ++i) nslots2 = std::max(nslots2, pt_node_slots(eoff[g] + i * n, n));
    }
    std::unique_ptr<int[]> d_na(new int[B]), d_n2g(new int[N]), d_rowptr(new int[N + 1]), d_ediag(new int[N]), d_src(new int[E]), d_dst(new int[E]),
        d_eg(new int[E]), d_pi(new int[Np]), d_pj(new int[Np]), d_e1(new int[Np]), d_e2(new int[Np]), d_pg(new int[Np]);
    PoolTables t{noff.get(),  eoff.get(), poff.get(), B,          d_na.get(), d_n2g.get(), d_rowptr.get(), d_ediag.get(),
                 d_src.get(), d_dst.get(), d_eg.get(), d_pi.get(), d_pj.get(), d_e1.get(),  d_e2.get(),     d_pg.get()};
    for (int g = 0; g < B; ++g) pt_crystal(t, g);
    for (int v = 0; v <= N; ++v) pt_node(t, v);
    for (int64_t k = 0; k < E; ++k) pt_edge(t, k);
    for (int64_t k = 0; k < Np; ++k) pt_pair(t, k);
    int bad = 0;
    auto cmp = [&](const char* name, const int* got, const std::vector<int>& want) {
        for (size_t k = 0; k < want.size(); ++k)
            if (got[k] != want[k]) {
                if (!bad) std::fprintf(stderr, "%s: %s[%zu] = %d, the host loops give %d\n", what, name, k, got[k], want[k]);
                ++bad;
                return;
            }
    };
    if (eoff[B] != (int)E || poff[B] != (int)Np || nslots2 != nslots) {
        std::fprintf(stderr, "%s: E %d / %lld, Np %d / %lld, nslots %d / %d\n", what, eoff[B], (long long)E, poff[B], (long long)Np, nslots2, nslots);
        ++bad;
    }
    cmp("num_atoms", d_na.get(), na);
    cmp("node2graph", d_n2g.get(), n2g);
    cmp("rowptr", d_rowptr.get(), rowptr);
    cmp("e_diag", d_ediag.get(), ediag);
    cmp("src", d_src.get(), src);
    cmp("dst", d_dst.get(), dst);
    cmp("edge_graph", d_eg.get(), egraph);
    cmp("pair_i", d_pi.get(), pr_i);
    cmp("pair_j", d_pj.get(), pr_j);
    cmp("pair_e1", d_e1.get(), pr_e1);
    cmp("pair_e2", d_e2.get(), pr_e2);
    cmp("pair_graph", d_pg.get(), pr_g);
    cmp("pair_off", poff.get(), pr_off);
    return bad;
}

int main() {
    int bad = 0, cases = 0;
    char name[64];
    for (int n = 1; n <= 200; ++n, ++cases) {
        std::snprintf(name, sizeof name, "[%d]", n);
        bad += check({n}, name);
    }
    bad += check({1, 7, 20, 3, 13}, "[1, 7, 20, 3, 13]");
    std::vector<int> cyc(300);
    for (int g = 0; g < 300; ++g) cyc[g] = 1 + g % 5;
    bad += check(cyc, "300 crystals cycling 1..5");
    bad += check({0, 4, 0, 0, 1, 2, 0}, "[0, 4, 0, 0, 1, 2, 0]");
    bad += check({3, 0}, "[3, 0]");
    cases += 4;
    std::printf("%d cases, %d mismatching table(s)\n", cases, bad);
    return bad ? 1 : 0;
}
