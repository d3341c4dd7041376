// The kernel of the symmetry constraint (matinvent_amd/csrc/sym_constraint.hip) run on the host: the same functions of
// matinvent_amd/csrc/sym_constraint.h in the kernel's order, with the workgroup and thread index as loop variables and the tree over LDS
// written as the same tree over a vector -- so that the host sanitizers see every index the kernel forms:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all scripts/sym_constraint_host_check.cpp -o sym_constraint_host_check
//   ./sym_constraint_host_check CASE.bin OUT.bin
//
// CASE.bin (little endian): int32 B, N, NR; then the constraint as the kernel reads it -- K [B] i32, roff [B + 1] i32, rot [NR][9] i32
// (the distinct rotation parts), rep [N] i32, node_off [B + 1] i32, Q [N][9] f64, d [N][3] f64 -- and the state: atom_types [N][100] f32,
// frac [N][3] f32, lattices [B][9] f32.  Every array is a heap block of exactly its size.  OUT.bin: atom_types, frac, lattices as the
// kernel leaves them, fail [B] i32 (from 0).  tests/test_symc_host.py writes the cases and compares every output with tests/symc_ref64.py
// bit for bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../matinvent_amd/csrc/sym_constraint.h"

using namespace mi;

template <typename T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "sym_constraint_host_check: short case file\n");
        exit(2);
    }
    return v;
}
template <typename T>
static void wr(FILE* f, const std::vector<T>& v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: sym_constraint_host_check CASE.bin OUT.bin\n");
        return 2;
    }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    const auto head = rd<int>(fi, 3);
    const int B = head[0], N = head[1], NR = head[2];
    const auto K = rd<int>(fi, (size_t)B);
    const auto roff = rd<int>(fi, (size_t)B + 1);
    const auto rot = rd<int>(fi, (size_t)NR * 9);
    const auto rep = rd<int>(fi, (size_t)N);
    const auto node_off = rd<int>(fi, (size_t)B + 1);
    const auto Q = rd<double>(fi, (size_t)N * 9);
    const auto d = rd<double>(fi, (size_t)N * 3);
    auto types = rd<float>(fi, (size_t)N * 100);
    auto frac = rd<float>(fi, (size_t)N * 3);
    auto lat = rd<float>(fi, (size_t)B * 9);
    fclose(fi);
    const int THREADS = SYMC_THREADS;
    std::vector<int> fail((size_t)B, 0);
    long projected = 0, rows = 0;
    for (int b = 0; b < B; ++b) {   // blockIdx.x
        if (K[(size_t)b] <= 1) continue;
        const int n0 = node_off[(size_t)b], n = node_off[(size_t)b + 1] - n0;
        const int r0 = roff[(size_t)b], R = roff[(size_t)b + 1] - r0;
        // the crystal's rotation parts as a block of exactly their size: a read past them is an error here
        std::vector<int> crot(rot.begin() + (size_t)r0 * 9, rot.begin() + (size_t)(r0 + R) * 9);
        std::vector<float> x((size_t)n * 3, 0.f);
        std::vector<int> s_rep((size_t)n, 0);
        std::vector<double> red((size_t)9 * THREADS, 0.0);
        // ---- the reads
        for (int tid = 0; tid < n; ++tid) {
            const int r = rep[(size_t)(n0 + tid)];
            s_rep[(size_t)tid] = r;
            float xr[3];
            for (int c = 0; c < 3; ++c) xr[c] = frac[(size_t)(n0 + r) * 3 + c];
            symc_coord(xr, Q.data() + (size_t)(n0 + tid) * 9, d.data() + (size_t)(n0 + tid) * 3, x.data() + (size_t)tid * 3);
        }
        for (int tid = 0; tid < THREADS; ++tid) {
            double G[9], Gk[9];
            symc_metric(lat.data() + (size_t)b * 9, G);
            symc_slot(crot.data(), R, tid, G, Gk);
            for (int e = 0; e < 9; ++e) red[(size_t)e * THREADS + tid] = Gk[e];
        }
        // ---- the tree
        for (int s = THREADS / 2; s >= 1; s >>= 1)
            for (int tid = 0; tid < s; ++tid)
                for (int e = 0; e < 9; ++e)
                    red[(size_t)e * THREADS + tid] = refine_tree_add(red[(size_t)e * THREADS + tid], red[(size_t)e * THREADS + tid + s]);
        // ---- the writes
        for (int tid = 0; tid < n; ++tid)
            for (int c = 0; c < 3; ++c) frac[(size_t)(n0 + tid) * 3 + c] = x[(size_t)tid * 3 + c];
        {
            double Gsum[9];
            float cell[9];
            for (int e = 0; e < 9; ++e) Gsum[e] = red[(size_t)e * THREADS];
            if (symc_cell(Gsum, R, cell)) {
                for (int e = 0; e < 9; ++e) lat[(size_t)b * 9 + e] = cell[e];
            } else {
                fail[(size_t)b] = fail[(size_t)b] + 1;
            }
        }
        for (int tid = 0; tid < THREADS; ++tid)
            for (int item = tid; item < n * SYMC_QUADS; item += THREADS) {
                const int j = item / SYMC_QUADS, q = item - j * SYMC_QUADS, r = s_rep[(size_t)j];
                if (r == j) continue;
                for (int e = 0; e < 4; ++e) types[(size_t)(n0 + j) * 100 + 4 * q + e] = types[(size_t)(n0 + r) * 100 + 4 * q + e];
                ++rows;
            }
        ++projected;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    wr(o, types), wr(o, frac), wr(o, lat), wr(o, fail);
    fclose(o);
    printf("sym_constraint_host_check: %d crystals, %ld projected, %ld row quads\n", B, projected, rows);
    return 0;
}
