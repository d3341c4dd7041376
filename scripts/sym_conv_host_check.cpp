// The kernels of the conventional cell (matinvent_amd/csrc/sym_conv.hip) run on the host: the same functions of matinvent_amd/csrc/sym_conv.h
// in the kernels' order, with the workgroup, lane and thread index as loop variables and the tree minimum of a search written as the serial
// minimum of (length, index) it equals -- so that the host sanitizers see every index the kernels form:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all scripts/sym_conv_host_check.cpp -o sym_conv_host_check
//   ./sym_conv_host_check CASE.bin OUT.bin
//
// CASE.bin (little endian): int32 B, N; then the prepared set of the primitive crystals and the find result of it, as the kernels read
// them: offsets [B + 1] i32, prepare info [B][4] i32, prepared cell [B][9] f64, types [N] i32, frac [N][3] f32, lat [B][9] f32, find info
// [B][8] i32, find rot [B][192][9] i32.  Every array is a heap block of exactly its size.
// OUT.bin: conv_info [B][8], conv_M [B][9], conv_cvec [B][4][3], conv_count [B], conv_offsets [B + 1], types [4 N] i32; frac [4 N][3],
// lat [B][9] f32.  Pre-filled with -7.  tests/test_conventional_host.py writes the cases and compares every output with
// tests/conv_ref64.py bit for bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../matinvent_amd/csrc/sym_conv.h"

using namespace mi;

template <typename T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "sym_conv_host_check: short case file\n");
        exit(2);
    }
    return v;
}
template <typename T>
static void wr(FILE* f, const std::vector<T>& v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

// the search of conv_basis as a serial loop in ascending index: the minimum of (length, index)
struct SerialSearch {
    const double* G;
    long* searches;
    int operator()(const int* S, const int* excl, bool use_excl) const {
        const int side = 2 * CONV_BOX + 1;
        double best = sm_inf();
        int bp = CONV_NO_POINT;
        for (int p = 0; p < side * side * side; ++p) {
            double l2;
            if (conv_cand(p, CONV_BOX, S, excl, use_excl, G, &l2) && sm_better(l2, p, best, bp)) best = l2, bp = p;
        }
        ++*searches;
        return bp == CONV_NO_POINT ? -1 : bp;
    }
};

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: sym_conv_host_check CASE.bin OUT.bin\n");
        return 2;
    }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    const auto head = rd<int>(fi, 2);
    const int B = head[0], N = head[1];
    const auto offsets = rd<int>(fi, (size_t)B + 1);
    const auto p_info = rd<int>(fi, (size_t)B * 4);
    const auto p_lat = rd<double>(fi, (size_t)B * 9);
    const auto types = rd<int>(fi, (size_t)N);
    const auto frac = rd<float>(fi, (size_t)N * 3), lat = rd<float>(fi, (size_t)B * 9);
    const auto s_info = rd<int>(fi, (size_t)B * SYM_INFO);
    const auto s_rot = rd<int>(fi, (size_t)B * SYM_MAX_OPS * 9);
    fclose(fi);
    const int POISON = -7;
    const size_t cap = (size_t)4 * (size_t)N;
    std::vector<int> c_info((size_t)B * CONV_INFO, POISON), c_M((size_t)B * 9, POISON), c_cvec((size_t)B * CONV_MAX_MULT * 3, POISON), c_count((size_t)B, POISON),
        c_off((size_t)B + 1, POISON), ws_adj((size_t)B * 9, POISON), o_types(cap, POISON);
    std::vector<float> o_frac(cap * 3, (float)POISON), o_lat((size_t)B * 9, (float)POISON);
    long searches = 0;
    auto fail = [&](int b, int n, int system, int n_axes, int status, bool cell) {
        const int row[CONV_INFO] = {0, CONV_NONE, 1, system, n_axes, 1, 0, status};
        for (int i = 0; i < CONV_INFO; ++i) c_info[(size_t)b * CONV_INFO + i] = row[i];
        for (int i = 0; i < 9; ++i) {
            c_M[(size_t)b * 9 + i] = ws_adj[(size_t)b * 9 + i] = i % 4 == 0 ? 1 : 0;
            if (cell) o_lat[(size_t)b * 9 + i] = lat[(size_t)b * 9 + i];
        }
        for (int i = 0; i < CONV_MAX_MULT * 3; ++i) c_cvec[(size_t)b * CONV_MAX_MULT * 3 + i] = 0;
        c_count[(size_t)b] = n;
    };
    // ---- sym_conv_basis_kernel: blockIdx.x = b
    for (int b = 0; b < B; ++b) {
        const int* sinfo = s_info.data() + (size_t)b * SYM_INFO;
        const int find_status = sinfo[SYM_INFO - 1], system = sinfo[5], nops = sinfo[0];
        const int* pinfo = p_info.data() + (size_t)b * 4;
        if (pinfo[3] != SM_PREP_OK) {
            fail(b, 0, 0, 0, find_status | SYM_NOT_PREPARED | SYM_CONV_FAIL, false);
            continue;
        }
        const int n = pinfo[0];
        if (find_status != SYM_OK || nops < 1 || nops > SYM_MAX_OPS) {
            fail(b, n, system, 0, find_status | SYM_CONV_FAIL, true);
            continue;
        }
        // the crystal's operations as a block of exactly nops rows: a read past them is an error here
        std::vector<int> rot(s_rot.begin() + (size_t)b * SYM_MAX_OPS * 9, s_rot.begin() + ((size_t)b * SYM_MAX_OPS + (size_t)nops) * 9);
        std::vector<int> order((size_t)nops), axis((size_t)nops * 3);
        for (int i = 0; i < nops; ++i) {   // a lane per operation
            int W[9], o = -1, ax[3] = {0, 0, 0};
            bool fresh = i == 0;
            for (int e = 0; e < 9; ++e) W[e] = rot[(size_t)9 * i + e], fresh = fresh || W[e] != rot[(size_t)9 * (i > 0 ? i - 1 : 0) + e];
            if (fresh) conv_classify(W, &o, ax);
            order[(size_t)i] = o, axis[(size_t)3 * i] = ax[0], axis[(size_t)3 * i + 1] = ax[1], axis[(size_t)3 * i + 2] = ax[2];
        }
        ConvAxes axes;
        conv_collect_begin(&axes);
        for (int i = 0; i < nops; ++i) conv_collect(&axes, i, order[(size_t)i], axis.data() + (size_t)3 * i);
        double G[9];
        sym_metric(p_lat.data() + (size_t)b * 9, G);
        int M[9], n_axes = 0, mult = 1, centring = CONV_NONE, bravais = 0;
        std::vector<int> cvec((size_t)CONV_MAX_MULT * 3, 0);
        const SerialSearch search{G, &searches};
        if (conv_basis(system, axes, rot.data(), G, CONV_BOX, search, M, &n_axes)) bravais = conv_finish(system, M, &mult, &centring, cvec.data());
        int T[9], adj[9];
        double L0[9], Lr[9];
        for (int i = 0; i < 9; ++i) L0[i] = (double)lat[(size_t)b * 9 + i];
        sm_reduce(L0, T, Lr);
        if (bravais == 0 || !conv_transform(M, T, adj)) {
            fail(b, n, system, n_axes, find_status | SYM_CONV_FAIL, true);
            continue;
        }
        const int row[CONV_INFO] = {bravais, centring, mult, system, n_axes, conv_max_abs(M), 0, find_status};
        for (int i = 0; i < CONV_INFO; ++i) c_info[(size_t)b * CONV_INFO + i] = row[i];
        for (int i = 0; i < 9; ++i) c_M[(size_t)b * 9 + i] = M[i], ws_adj[(size_t)b * 9 + i] = adj[i];
        for (int i = 0; i < CONV_MAX_MULT * 3; ++i) c_cvec[(size_t)b * CONV_MAX_MULT * 3 + i] = cvec[(size_t)i];
        for (int i = 0; i < 3; ++i) {
            double r[3];
            conv_lat_row(M, Lr, i, r);
            for (int c = 0; c < 3; ++c) o_lat[(size_t)b * 9 + 3 * i + c] = (float)r[c];
        }
        c_count[(size_t)b] = mult * n;
    }
    // ---- sym_conv_scan_kernel
    c_off[0] = 0;
    for (int b = 0; b < B; ++b) c_off[(size_t)b + 1] = c_off[(size_t)b] + c_count[(size_t)b];
    // ---- sym_conv_gather_kernel: a thread per output row
    long atoms = 0;
    for (int64_t t64 = 0; B > 0 && t64 < (int64_t)4 * N; ++t64) {
        const int total = c_off[(size_t)B];
        if (t64 >= (int64_t)total) break;
        const int t = (int)t64;
        int lo = 0, hi = B - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (c_off[(size_t)mid + 1] > t) hi = mid;
            else lo = mid + 1;
        }
        const int b = lo, r = t - c_off[(size_t)b];
        const int* info = c_info.data() + (size_t)b * CONV_INFO;
        const int mult = info[2];
        const int n0 = offsets[(size_t)b], n = p_info[(size_t)b * 4];
        if (r < 0 || mult < 1 || mult > CONV_MAX_MULT) continue;
        const int i = r / mult, j = r - i * mult;
        if (i >= n) continue;
        const float* f = frac.data() + (size_t)(n0 + i) * 3;
        o_types[(size_t)t] = types[(size_t)(n0 + i)];
        ++atoms;
        if (info[0] == 0) {
            for (int c = 0; c < 3; ++c) o_frac[(size_t)t * 3 + c] = f[c];
            continue;
        }
        conv_frac(f, ws_adj.data() + (size_t)b * 9, c_cvec.data() + ((size_t)b * CONV_MAX_MULT + (size_t)j) * 3, mult, o_frac.data() + (size_t)t * 3);
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    wr(o, c_info), wr(o, c_M), wr(o, c_cvec), wr(o, c_count), wr(o, c_off), wr(o, o_types), wr(o, o_frac), wr(o, o_lat);
    fclose(o);
    printf("sym_conv_host_check: %d crystals, %ld searches, %ld atoms written\n", B, searches, atoms);
    return 0;
}
