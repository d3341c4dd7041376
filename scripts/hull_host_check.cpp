// The two kernels of mi_hull_above (matinvent_amd/csrc/hull.hip) run on the host: the same per-thread functions of
// matinvent_amd/csrc/hull_simplex.h, in the kernels' order, with the workgroup index and the thread index as loop variables and the
// wave butterfly and the four-wave fold of the argmin written out -- so that the host sanitizers see every index the kernels form:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all scripts/hull_host_check.cpp -o hull_host_check
//   ./hull_host_check CASE.bin OUT.bin
//
// CASE.bin (little endian): int32 M, G, Q, nnz_q, nnz_c, no_lds; then bank_nelem [M] i32, bank_Z [M][8] i32, bank_frac [M][8] f64,
// bank_energy [M] f64, grp_nelem [G] i32, grp_Z [G][8] i32, grp_q_off [G + 1] i32, q_idx [nnz_q] i32, grp_c_off [G + 1] i32,
// c_idx [nnz_c] i32, query_c [Q][8] f64, query_e [Q] f64.  Every array is a heap block of exactly its size.
// OUT.bin: e_hull [Q], e_above [Q], chempot [Q][8], decomp_frac [Q][8] f64, then decomp_idx [Q][8], iters [Q], status [Q], flags [Q] i32,
// pre-filled as the Python caller pre-fills them (NaN / 0 / -1 / 0 / -1 / 0), so that a row no group owns is visible.
// tests/test_hull_host.py writes the cases and compares every output with tests/hull_ref64.py bit for bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../matinvent_amd/csrc/hull_simplex.h"

using namespace mi;

template <typename T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "hull_host_check: short case file\n");
        exit(2);
    }
    return v;
}
template <typename T>
static void wr(FILE* f, const std::vector<T>& v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

// hull_block_argmin of hull.hip: per wave the xor butterfly 32, 16, .., 1; then the waves in order
static void block_argmin(std::vector<double>& v, std::vector<int>& p, double& bv, int& bp) {
    const int T = HULL_THREADS;
    for (int m = 32; m >= 1; m >>= 1) {
        std::vector<double> nv = v;
        std::vector<int> np = p;
        for (int t = 0; t < T; ++t) {
            const int o = (t & ~63) | ((t & 63) ^ m);
            if (hull_better(v[(size_t)o], p[(size_t)o], v[(size_t)t], p[(size_t)t])) nv[(size_t)t] = v[(size_t)o], np[(size_t)t] = p[(size_t)o];
        }
        v = nv, p = np;
    }
    bv = v[0], bp = p[0];
    for (int w = 1; w < T / 64; ++w)
        if (hull_better(v[(size_t)w * 64], p[(size_t)w * 64], bv, bp)) bv = v[(size_t)w * 64], bp = p[(size_t)w * 64];
}

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: hull_host_check CASE.bin OUT.bin\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int> head = rd<int>(f, 6);
    const int M = head[0], G = head[1], Q = head[2], nnz_q = head[3], nnz_c = head[4], no_lds = head[5];
    const auto bank_nelem = rd<int>(f, (size_t)M), bank_Z = rd<int>(f, (size_t)M * 8);
    const auto bank_frac = rd<double>(f, (size_t)M * 8), bank_energy = rd<double>(f, (size_t)M);
    const auto grp_nelem = rd<int>(f, (size_t)G), grp_Z = rd<int>(f, (size_t)G * 8), grp_q_off = rd<int>(f, (size_t)G + 1), q_idx = rd<int>(f, (size_t)nnz_q);
    const auto grp_c_off = rd<int>(f, (size_t)G + 1), c_idx = rd<int>(f, (size_t)nnz_c);
    const auto query_c = rd<double>(f, (size_t)Q * 8), query_e = rd<double>(f, (size_t)Q);
    fclose(f);
    const int T = HULL_THREADS;
    std::vector<double> e_hull((size_t)Q, hull_nan()), e_above((size_t)Q, hull_nan()), chempot((size_t)Q * 8, hull_nan()), decomp_frac((size_t)Q * 8, 0.0);
    std::vector<int> decomp_idx((size_t)Q * 8, -1), iters((size_t)Q, 0), status((size_t)Q, -1), flags((size_t)Q, 0);
    // the workspace
    std::vector<double> ws_x((size_t)nnz_c * HULL_COLS, 0.0);
    std::vector<int> ws_row((size_t)nnz_c, 0), ws_qgrp((size_t)nnz_q, -1), ws_gflag((size_t)G, 0);
    const HullBank bank{bank_nelem.data(), bank_Z.data(), bank_frac.data(), bank_energy.data(), M};
    long staged = 0, skipped_n = 0, lds_n = 0, stream_n = 0;
    // ---- hull_stage_kernel: blockIdx.x = g, threadIdx.x = tid
    for (int g = 0; g < G; ++g) {
        const int d = grp_nelem[(size_t)g];
        const int* gZ = grp_Z.data() + (size_t)g * HULL_MAX_ELEMS;
        const int q0 = grp_q_off[(size_t)g], q1 = grp_q_off[(size_t)g + 1], c0 = grp_c_off[(size_t)g], c1 = grp_c_off[(size_t)g + 1];
        if (!(hull_group_ok(gZ, d) && q0 >= 0 && q0 <= q1 && q1 <= nnz_q && c0 >= 0 && c0 <= c1 && c1 <= nnz_c)) continue;
        const int nc = c1 - c0;
        int skipped = 0;
        for (int tid = 0; tid < T; ++tid) {
            for (int i = tid; i < nc; i += T) {
                skipped |= hull_stage_candidate(bank, gZ, d, c_idx[(size_t)(c0 + i)], ws_x.data() + (size_t)HULL_COLS * c0, ws_row.data() + c0, nc, i);
                ++staged;
            }
            for (int p = q0 + tid; p < q1; p += T) ws_qgrp[(size_t)p] = g;
        }
        ws_gflag[(size_t)g] = skipped ? HULL_FLAG_SKIPPED : 0;
        skipped_n += skipped;
    }
    // ---- hull_solve_kernel: blockIdx.x = pos, threadIdx.x = tid
    for (int pos = 0; pos < nnz_q; ++pos) {
        const int g = ws_qgrp[(size_t)pos];
        if (g < 0 || g >= G) continue;
        const int q = q_idx[(size_t)pos];
        if (q < 0 || q >= Q) continue;
        const int d = grp_nelem[(size_t)g], c0 = grp_c_off[(size_t)g], nc = grp_c_off[(size_t)g + 1] - c0;
        const double* gx = ws_x.data() + (size_t)HULL_COLS * c0;
        const int* rows = ws_row.data() + c0;
        const int64_t cells = (int64_t)(d + 1) * nc;
        const bool in_lds = !no_lds && cells <= HULL_LDS_DOUBLES;
        std::vector<double> lds(in_lds ? (size_t)cells : 0);   // (exactly the cells that the kernel copies)
        for (int tid = 0; tid < T; ++tid)
            for (int i = tid; i < (int)lds.size(); i += T) lds[(size_t)i] = gx[i];
        (in_lds ? lds_n : stream_n)++;
        HullState s;
        memset(&s, 0, sizeof(s));
        for (int tid = 0; tid < HULL_MAX_ELEMS; ++tid) s.c[tid] = tid < d ? query_c[(size_t)q * HULL_MAX_ELEMS + tid] : 0.0;
        const HullBlock blk{in_lds ? lds.data() : gx, rows, nc, d};
        std::vector<double> v((size_t)T);
        std::vector<int> p((size_t)T);
        for (int k = 0; k < d; ++k) {
            for (int tid = 0; tid < T; ++tid) hull_terminal_thread(blk, k, tid, T, v[(size_t)tid], p[(size_t)tid]);
            double bv;
            int bp;
            block_argmin(v, p, bv, bp);
            s.basis[k] = bp, s.EB[k] = bv;
        }
        hull_start(s, d);
        while (!s.done) {
            double y[HULL_MAX_ELEMS];
            int basis[HULL_MAX_ELEMS];
            for (int k = 0; k < HULL_MAX_ELEMS; ++k) {
                y[k] = k < d ? s.y[k] : 0.0;
                basis[k] = k < d ? s.basis[k] : -1;
            }
            for (int tid = 0; tid < T; ++tid) hull_price_thread(blk, y, basis, tid, T, v[(size_t)tid], p[(size_t)tid]);
            double rmin;
            int j;
            block_argmin(v, p, rmin, j);
            double Ej = 0.0;
            if (j != HULL_NO_POS) {
                for (int k = 0; k < d; ++k) s.xj[k] = hull_block_frac(blk, j, k);
                Ej = hull_block_energy(blk, j);
            }
            hull_decide(s, rmin, j, Ej);
        }
        const bool solved = s.status != HULL_NO_TERMINAL && s.status != HULL_BAD_QUERY;
        for (int tid = 0; tid < HULL_MAX_ELEMS; ++tid) {
            const bool live = solved && tid < d;
            chempot[(size_t)q * HULL_MAX_ELEMS + tid] = solved ? (tid < d ? s.y[tid] : 0.0) : hull_nan();
            decomp_frac[(size_t)q * HULL_MAX_ELEMS + tid] = live ? s.lam[tid] : 0.0;
            decomp_idx[(size_t)q * HULL_MAX_ELEMS + tid] = live ? rows[s.basis[tid]] : -1;
        }
        const double eh = solved ? hull_value(s) : hull_nan();
        e_hull[(size_t)q] = eh;
        e_above[(size_t)q] = query_e[(size_t)q] - eh;
        iters[(size_t)q] = s.iters;
        status[(size_t)q] = s.status;
        flags[(size_t)q] = ws_gflag[(size_t)g];
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    wr(o, e_hull), wr(o, e_above), wr(o, chempot), wr(o, decomp_frac), wr(o, decomp_idx), wr(o, iters), wr(o, status), wr(o, flags);
    fclose(o);
    printf("hull_host_check: %d groups, %d query positions, %ld candidates staged, %ld groups with a skipped candidate, %ld blocks in LDS, %ld streamed\n", G,
           nnz_q, staged, skipped_n, lds_n, stream_n);
    return 0;
}
