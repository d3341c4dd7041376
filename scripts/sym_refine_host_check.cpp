// The kernel of the refined structure (matinvent_amd/csrc/sym_refine.hip) run on the host: the same functions of
// matinvent_amd/csrc/sym_refine.h in the kernel's order, with the workgroup and thread index as loop variables and the trees over LDS
// written as the same trees over a vector -- so that the host sanitizers see every index the kernel forms:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all scripts/sym_refine_host_check.cpp -o sym_refine_host_check
//   ./sym_refine_host_check CASE.bin OUT.bin
//
// CASE.bin (little endian): int32 B, N; then the prepared set and the find result of it, as the kernel reads them: offsets [B + 1] i32,
// prepare info [B][4] i32, prepared cell [B][9] f64, prepared frac [N][3] f64, perm [N] i32, spec_off [B][17] i32, frac [N][3] f32, lat
// [B][9] f32, find info [B][8] i32, find rot [B][192][9] i32, find trans [B][192][3] f64.  Every array is a heap block of exactly its size.
// OUT.bin: refine_info [B][8] i32, refine_stat [B][4] f64, orbit, mult, site_order [N] i32, trans_ref [B][192][3] f64, frac [N][3] f32, lat
// [B][9] f32.  Pre-filled with -7.  tests/test_refine_host.py writes the cases and compares every output with tests/refine_ref64.py bit
// for bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../matinvent_amd/csrc/sym_refine.h"

using namespace mi;

template <typename T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "sym_refine_host_check: short case file\n");
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
        fprintf(stderr, "usage: sym_refine_host_check CASE.bin OUT.bin\n");
        return 2;
    }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    const auto head = rd<int>(fi, 2);
    const int B = head[0], N = head[1];
    const auto offsets = rd<int>(fi, (size_t)B + 1);
    const auto p_info = rd<int>(fi, (size_t)B * 4);
    const auto p_lat = rd<double>(fi, (size_t)B * 9);
    const auto p_frac = rd<double>(fi, (size_t)N * 3);
    const auto p_perm = rd<int>(fi, (size_t)N);
    const auto p_spec = rd<int>(fi, (size_t)B * (SM_MAX_SPECIES + 1));
    const auto frac = rd<float>(fi, (size_t)N * 3), lat = rd<float>(fi, (size_t)B * 9);
    const auto s_info = rd<int>(fi, (size_t)B * SYM_INFO);
    const auto s_rot = rd<int>(fi, (size_t)B * SYM_MAX_OPS * 9);
    const auto s_trans = rd<double>(fi, (size_t)B * SYM_MAX_OPS * 3);
    fclose(fi);
    const int POISON = -7, THREADS = SM_THREADS;
    std::vector<int> r_info((size_t)B * REFINE_INFO, POISON), orbit((size_t)N, POISON), mult((size_t)N, POISON), site((size_t)N, POISON);
    std::vector<double> r_stat((size_t)B * REFINE_STAT, (double)POISON), trans_ref((size_t)B * SYM_MAX_OPS * 3, (double)POISON);
    std::vector<float> o_frac((size_t)N * 3, (float)POISON), o_lat((size_t)B * 9, (float)POISON);
    long items = 0, refined = 0;
    auto rows = [&](int b, int n_orbits, int n_ops, int status) {
        for (int t = 0; t < REFINE_INFO; ++t) r_info[(size_t)b * REFINE_INFO + t] = t == 0 ? n_orbits : (t == 1 ? n_ops : (t == REFINE_INFO - 1 ? status : 0));
        for (int t = 0; t < REFINE_STAT; ++t) r_stat[(size_t)b * REFINE_STAT + t] = 0.0;
    };
    auto copy = [&](int b, int n0, int n, int n_ops, int status) {
        for (int i = 0; i < n; ++i) {
            for (int c = 0; c < 3; ++c) o_frac[(size_t)(n0 + i) * 3 + c] = frac[(size_t)(n0 + i) * 3 + c];
            orbit[(size_t)(n0 + i)] = i, mult[(size_t)(n0 + i)] = 1, site[(size_t)(n0 + i)] = 1;
        }
        for (int e = 0; e < 9; ++e) o_lat[(size_t)b * 9 + e] = lat[(size_t)b * 9 + e];
        rows(b, n, n_ops, status);
    };
    for (int b = 0; b < B; ++b) {   // blockIdx.x
        const int* sinfo = s_info.data() + (size_t)b * SYM_INFO;
        const int find_status = sinfo[SYM_INFO - 1], nops = sinfo[0];
        const int* pinfo = p_info.data() + (size_t)b * 4;
        const int n = pinfo[0], nspec = pinfo[1];
        if (pinfo[3] != SM_PREP_OK || n < 1 || n > SM_MAX_ATOMS || nspec < 1 || nspec > SM_MAX_SPECIES) {
            rows(b, 0, 0, find_status | SYM_NOT_PREPARED | SYM_REFINE_FAIL);
            continue;
        }
        const int n0 = offsets[(size_t)b];
        if (find_status != SYM_OK || nops < 1 || nops > SYM_MAX_OPS) {
            copy(b, n0, n, nops, find_status | SYM_REFINE_FAIL);
            continue;
        }
        if (nops == 1) {
            copy(b, n0, n, 1, find_status);
            continue;
        }
        // the crystal as blocks of exactly their sizes: a read past them is an error here
        const int* spec_off = p_spec.data() + (size_t)b * (SM_MAX_SPECIES + 1);
        std::vector<double> f(p_frac.begin() + (size_t)n0 * 3, p_frac.begin() + (size_t)(n0 + n) * 3);
        std::vector<int> rot(s_rot.begin() + (size_t)b * SYM_MAX_OPS * 9, s_rot.begin() + ((size_t)b * SYM_MAX_OPS + (size_t)nops) * 9);
        std::vector<double> t(s_trans.begin() + (size_t)b * SYM_MAX_OPS * 3, s_trans.begin() + ((size_t)b * SYM_MAX_OPS + (size_t)nops) * 3);
        std::vector<int> perm((size_t)n), blk0((size_t)n), blkn((size_t)n), v_bad((size_t)THREADS, 0), v_cnt((size_t)THREADS, 0);
        std::vector<unsigned char> sig((size_t)(nops - 1) * REFINE_ROW + (size_t)n, 255);
        std::vector<double> tbar((size_t)nops * 3), d2max((size_t)THREADS, 0.0);
        std::vector<double> red0((size_t)THREADS, 0.0), red1((size_t)THREADS, 0.0), red2((size_t)THREADS, 0.0);
        bool early = false;
        for (int tid = 0; tid < n; ++tid) {
            int b0, nb;
            refine_block(spec_off, nspec, tid, &b0, &nb);
            const int p = p_perm[(size_t)(n0 + tid)];
            const bool bad = b0 < 0 || nb < 1 || b0 + nb > n || tid < b0 || tid >= b0 + nb || p < 0 || p >= n;
            blk0[(size_t)tid] = b0, blkn[(size_t)tid] = nb, perm[(size_t)tid] = bad ? 0 : p;
            early = early || bad;
        }
        if (early) {
            copy(b, n0, n, nops, find_status | SYM_REFINE_FAIL);
            continue;
        }
        double G[9];
        sym_metric(p_lat.data() + (size_t)b * 9, G);
        // ---- A
        for (int tid = 0; tid < THREADS; ++tid)
            for (int item = tid; item < nops * n; item += THREADS) {
                const int k = item / n, i = item - k * n;
                double d2;
                const int at = refine_sigma(G, f.data(), blk0[(size_t)i], blkn[(size_t)i], i, rot.data() + (size_t)9 * k, t.data() + (size_t)3 * k, &d2);
                sig[(size_t)REFINE_ROW * k + i] = (unsigned char)at;
                d2max[(size_t)tid] = refine_max(d2max[(size_t)tid], d2);
                ++items;
            }
        // ---- B
        int T[9];
        float cell[9];
        double Gbar[9], change = 0.0;
        for (int tid = 0; tid < nops; ++tid) {
            v_bad[(size_t)tid] = refine_bijection(sig.data() + (size_t)REFINE_ROW * tid, n) ? 0 : 1;
            refine_translation(G, f.data(), n, sig.data() + (size_t)REFINE_ROW * tid, rot.data() + (size_t)9 * tid, t.data() + (size_t)3 * tid, tbar.data() + (size_t)3 * tid);
        }
        if (!refine_cell(lat.data() + (size_t)b * 9, rot.data(), nops, T, Gbar, &change, cell)) v_bad[(size_t)THREADS - 1] = 1;
        // ---- C
        std::vector<double> xbar((size_t)n * 3);
        std::vector<int> low((size_t)n), mu((size_t)n), stab((size_t)n);
        for (int tid = 0; tid < n; ++tid) {
            double q;
            refine_site(G, f.data(), tid, sig.data(), rot.data(), tbar.data(), nops, perm.data(), xbar.data() + (size_t)3 * tid, &q, &low[(size_t)tid], &mu[(size_t)tid],
                        &stab[(size_t)tid]);
            if (mu[(size_t)tid] * stab[(size_t)tid] != nops) v_bad[(size_t)tid] = 1;
            v_cnt[(size_t)tid] = low[(size_t)tid] == perm[(size_t)tid] ? 1 : 0;
            red0[(size_t)tid] = q, red1[(size_t)tid] = q;
        }
        for (int tid = 0; tid < THREADS; ++tid) red2[(size_t)tid] = d2max[(size_t)tid];
        for (int s = THREADS / 2; s >= 1; s >>= 1)
            for (int tid = 0; tid < s; ++tid) {
                v_bad[(size_t)tid] |= v_bad[(size_t)(tid + s)], v_cnt[(size_t)tid] += v_cnt[(size_t)(tid + s)];
                red0[(size_t)tid] = refine_max(red0[(size_t)tid], red0[(size_t)(tid + s)]);
                red1[(size_t)tid] = refine_tree_add(red1[(size_t)tid], red1[(size_t)(tid + s)]);
                red2[(size_t)tid] = refine_max(red2[(size_t)tid], red2[(size_t)(tid + s)]);
            }
        if (v_bad[0]) {
            copy(b, n0, n, nops, find_status | SYM_REFINE_FAIL);
            continue;
        }
        for (int tid = 0; tid < n; ++tid) {
            const int at = n0 + perm[(size_t)tid];
            refine_frac(xbar.data() + (size_t)3 * tid, T, o_frac.data() + (size_t)at * 3);
            orbit[(size_t)at] = low[(size_t)tid], mult[(size_t)at] = mu[(size_t)tid], site[(size_t)at] = stab[(size_t)tid];
        }
        for (int e = 0; e < 9; ++e) o_lat[(size_t)b * 9 + e] = cell[e];
        for (int i = 0; i < 3 * nops; ++i) trans_ref[(size_t)b * SYM_MAX_OPS * 3 + i] = tbar[(size_t)i];
        for (int tid = 0; tid < REFINE_INFO; ++tid) r_info[(size_t)b * REFINE_INFO + tid] = tid == 0 ? v_cnt[0] : (tid == 1 ? nops : (tid == REFINE_INFO - 1 ? find_status : 0));
        refine_stats(red0[0], red1[0], n, change, red2[0], r_stat.data() + (size_t)b * REFINE_STAT);
        ++refined;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    wr(o, r_info), wr(o, r_stat), wr(o, orbit), wr(o, mult), wr(o, site), wr(o, trans_ref), wr(o, o_frac), wr(o, o_lat);
    fclose(o);
    printf("sym_refine_host_check: %d crystals, %ld refined, %ld items\n", B, refined, items);
    return 0;
}
