// The kernels of the substrate matcher (matinvent_amd/csrc/zsl.hip) run on the host: the same functions of matinvent_amd/csrc/zsl_match.h,
// in the kernels' order, with the workgroup and thread index as loop variables, the per-thread state of the search kept in arrays of 256
// and the fixed tree (a butterfly inside each wave, then the four wave results in wave order) written out -- so that the host sanitizers
// see every index the kernels form:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all scripts/zsl_host_check.cpp -o zsl_host_check
//   ./zsl_host_check CASE.bin OUT.bin
//
// CASE.bin (little endian): int32 B, Pf, Ps, S, count; float64 max_area, max_area_ratio_tol, max_length_tol, max_angle_tol; film lat [B][9]
// f32; film hkl [Pf][3] i32; substrate lat [S][9] f32; plane hkl [Ps][3], cell_of [Ps], sub_off [S + 1] i32.  Every array is a heap block of
// exactly its size.
// OUT.bin: for the films' B Pf planes, then for the bank's Ps: vec [T][6], area [T] f64, mult [T], status [T] i32; s_table [Ps][3276][3]
// f64; res_d [B][Ps][10] f64, res_i [B][Ps][20] i32, res_n [B][Ps] i64; mcia [B][S] f64, mcia_plane, mcia_status [B][S] i32.  Pre-filled
// with -7.  tests/test_zsl_host.py writes the cases and compares with tests/zsl_ref64.py: integers and areas bit for bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../matinvent_amd/csrc/zsl_match.h"

using namespace mi;

template <typename T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "zsl_host_check: short case file\n");
        exit(2);
    }
    return v;
}
template <typename T>
static void wr(FILE* f, const std::vector<T>& v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

static constexpr ZslCounts COUNTS = zsl_counts();
static constexpr int THREADS = ZSL_THREADS, WAVES = ZSL_THREADS / 64;

struct Planes {
    std::vector<double> vec, area;
    std::vector<int> mult, status;
    explicit Planes(size_t T) : vec(T * 6, -7.0), area(T, -7.0), mult(T, -7), status(T, -7) {}
};

// zsl_planes_kernel: a thread per plane
static void planes_kernel(const std::vector<float>& lat, int C, const std::vector<int>& hkl, int P, const int* cell_of, double max_area, Planes& out) {
    const size_t T = cell_of ? (size_t)P : (size_t)C * P;
    for (size_t t = 0; t < T; ++t) {
        int cell, p;
        if (cell_of) {
            cell = cell_of[t], p = (int)t;
        } else {
            cell = (int)(t / (size_t)P), p = (int)(t - (size_t)cell * P);
        }
        double vec[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, area = 0.0;
        int mult = 0, status = ZSL_BAD_CELL;
        if (cell >= 0 && cell < C) status = zsl_plane(lat.data() + (size_t)cell * 9, hkl.data() + (size_t)p * 3, max_area, vec, &area, &mult);
        for (int i = 0; i < 6; ++i) out.vec[t * 6 + i] = vec[i];
        out.area[t] = area, out.mult[t] = mult, out.status[t] = status;
    }
}

static int clamp_mult(int m) { return m < 0 ? 0 : m > ZSL_MAX_MULT ? ZSL_MAX_MULT : m; }
static int clamp_status(int s) { return s < ZSL_OK || s > ZSL_BAD_CELL ? ZSL_BAD_CELL : s; }

// the butterfly of a wave: after it every lane holds the wave's result; `op(mine, other)` returns the kept one
template <typename V, typename Op>
static void butterfly(std::vector<V>& v, Op op) {
    for (int mk = 32; mk >= 1; mk >>= 1) {
        std::vector<V> nxt(v.size());
        for (size_t t = 0; t < v.size(); ++t) nxt[t] = op(v[t], v[(t & ~(size_t)63) | ((t & 63) ^ (size_t)mk)]);
        v = nxt;
    }
}

struct Best {
    double v;
    int k;
};

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: zsl_host_check CASE.bin OUT.bin\n");
        return 2;
    }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    const auto head = rd<int>(fi, 5);
    const auto par = rd<double>(fi, 4);
    const int B = head[0], Pf = head[1], Ps = head[2], S = head[3], count = head[4];
    const double max_area = par[0], rtol = par[1], ltol = par[2], atol = par[3];
    const auto f_lat = rd<float>(fi, (size_t)B * 9);
    const auto f_hkl = rd<int>(fi, (size_t)Pf * 3);
    const auto s_lat = rd<float>(fi, (size_t)S * 9);
    const auto s_hkl = rd<int>(fi, (size_t)Ps * 3), cell_of = rd<int>(fi, (size_t)Ps), sub_off = rd<int>(fi, (size_t)S + 1);
    fclose(fi);
    if (B < 0 || Pf < 1 || Ps < 0 || S < 0) return 2;

    Planes fp_((size_t)B * Pf), sp_((size_t)Ps);
    planes_kernel(f_lat, B, f_hkl, Pf, nullptr, max_area, fp_);
    planes_kernel(s_lat, S, s_hkl, Ps, cell_of.data(), max_area, sp_);

    // ---- zsl_tables_kernel: a workgroup per plane, a thread per entry
    std::vector<double> table((size_t)Ps * ZSL_TABLE * 3, -7.0);
    for (int t = 0; t < Ps; ++t) {
        const int st = clamp_status(sp_.status[(size_t)t]);
        if (st == ZSL_BAD_CELL) continue;
        const int m = clamp_mult(sp_.mult[(size_t)t]);
        const int entries = m >= 1 ? COUNTS.off[m + 1] : 0;
        bool any = false;
        for (int tid = 0; tid < THREADS; ++tid)
            for (int e = tid; e < entries; e += THREADS) {
                int n = 1;
                while (COUNTS.off[n + 1] <= e) ++n;
                int i, j, w;
                zsl_hnf(n, e - COUNTS.off[n], &i, &j, &w);
                double out[3];
                any = !zsl_super(sp_.vec.data() + (size_t)t * 6, i, j, w, out) || any;
                for (int c = 0; c < 3; ++c) table[((size_t)t * ZSL_TABLE + (size_t)e) * 3 + (size_t)c] = out[c];
            }
        if (any) sp_.status[(size_t)t] = zsl_max(st, ZSL_REDUCE_CAP);
    }

    // ---- zsl_search_kernel: a workgroup per (film, film plane, substrate plane)
    const size_t items = (size_t)B * Pf * Ps;
    std::vector<double> item_d(items * ZSL_ROW_D, -7.0);
    std::vector<int> item_i(items * ZSL_ROW_I, -7);
    std::vector<int64_t> item_n(items, -7);
    for (size_t item = 0; item < items; ++item) {
        const int sp = (int)(item % (size_t)Ps), fp = (int)((item / (size_t)Ps) % (size_t)Pf);
        const size_t fpl = item / (size_t)Ps;
        double* d = item_d.data() + item * ZSL_ROW_D;
        int* r = item_i.data() + item * ZSL_ROW_I;
        const int fst = clamp_status(fp_.status[fpl]), sst = clamp_status(sp_.status[(size_t)sp]);
        const double* vec = fp_.vec.data() + fpl * 6;
        const double* tab = table.data() + (size_t)sp * ZSL_TABLE * 3;
        if (fst == ZSL_BAD_CELL || sst == ZSL_BAD_CELL) {
            zsl_write_match(ZSL_NO_KEY, fp, vec, 0.0, tab, COUNTS.off, ltol, atol, d, r + 1);
            d[4] = zsl_inf();
            zsl_write_match(ZSL_NO_KEY, fp, vec, 0.0, tab, COUNTS.off, ltol, atol, d + 5, r + 10);
            d[9] = 0.0, r[0] = ZSL_BAD_CELL, r[19] = 0;
            item_n[item] = count ? 0 : -1;
            continue;
        }
        const int mf = clamp_mult(fp_.mult[fpl]), ms = clamp_mult(sp_.mult[(size_t)sp]);
        const double Af = fp_.area[fpl], As = sp_.area[(size_t)sp];
        std::vector<double> s_film((size_t)ZSL_MAX_HNF * 3);
        std::vector<int> s_adm((size_t)ZSL_MAX_MULT + 1, 0);
        std::vector<Best> best((size_t)THREADS, Best{zsl_inf(), ZSL_NO_KEY});
        std::vector<long long> matches((size_t)THREADS, 0);
        int lowest = ZSL_NO_KEY;
        bool cap = false;
        for (int nf = 1; nf <= mf; ++nf) {
            const int sig_f = COUNTS.sig[nf];
            for (int tid = 0; tid < THREADS; ++tid) {
                for (int h = tid; h < sig_f; h += THREADS) {
                    int i, j, w;
                    zsl_hnf(nf, h, &i, &j, &w);
                    double e[3];
                    cap = !zsl_super(vec, i, j, w, e) || cap;
                    for (int c = 0; c < 3; ++c) s_film[(size_t)(3 * h + c)] = e[c];
                }
                if (tid >= 1 && tid <= ms) s_adm[(size_t)tid] = zsl_admissible(Af, As, nf, tid, rtol) ? 1 : 0;
            }
            std::vector<int> key((size_t)THREADS, ZSL_NO_KEY);
            for (int ns = 1; ns <= ms; ++ns) {
                if (!s_adm[(size_t)ns]) continue;
                const int sig_s = COUNTS.sig[ns], pairs = sig_f * sig_s;
                const double* sub = tab + 3 * (size_t)COUNTS.off[ns];
                for (int tid = 0; tid < THREADS; ++tid)
                    for (int t = tid; t < pairs; t += THREADS) {
                        const int h = t / sig_s, g = t - h * sig_s;
                        double s[3];
                        if (zsl_match(s_film.data() + 3 * (size_t)h, sub + 3 * (size_t)g, ltol, atol, s)) {
                            const int k = zsl_key(nf, h, ns, g);
                            key[(size_t)tid] = k < key[(size_t)tid] ? k : key[(size_t)tid];
                            if (count) {
                                ++matches[(size_t)tid];
                                const double strain = zsl_strain(s);
                                Best& bt = best[(size_t)tid];
                                if (zsl_better(strain, k, bt.v, bt.k)) bt.v = strain, bt.k = k;
                            }
                        }
                    }
            }
            if (lowest == ZSL_NO_KEY) {
                butterfly(key, [](int a, int b) { return b < a ? b : a; });
                lowest = key[0];
                for (int w = 1; w < WAVES; ++w) lowest = key[(size_t)w * 64] < lowest ? key[(size_t)w * 64] : lowest;
                if (lowest != ZSL_NO_KEY && !count) break;
            }
        }
        long long n = 0;
        Best bb{zsl_inf(), ZSL_NO_KEY};
        if (count) {
            butterfly(matches, [](long long a, long long b) { return a + b; });
            for (int w = 0; w < WAVES; ++w) n += matches[(size_t)w * 64];
            butterfly(best, [](Best a, Best b) { return zsl_better(b.v, b.k, a.v, a.k) ? b : a; });
            bb = best[0];
            for (int w = 1; w < WAVES; ++w)
                if (zsl_better(best[(size_t)w * 64].v, best[(size_t)w * 64].k, bb.v, bb.k)) bb = best[(size_t)w * 64];
        }
        r[0] = zsl_max(zsl_max(fst, sst), cap ? ZSL_REDUCE_CAP : ZSL_OK);
        zsl_write_match(lowest, fp, vec, Af, tab, COUNTS.off, ltol, atol, d, r + 1);
        d[4] = count && bb.k != ZSL_NO_KEY ? bb.v : zsl_inf();
        zsl_write_match(count ? bb.k : ZSL_NO_KEY, fp, vec, Af, tab, COUNTS.off, ltol, atol, d + 5, r + 10);
        d[9] = 0.0, r[19] = 0;
        item_n[item] = count ? n : -1;
    }

    // ---- zsl_reduce_kernel: a thread per (film, substrate plane); zsl_mcia_kernel: a thread per (film, substrate)
    std::vector<double> res_d((size_t)B * Ps * ZSL_ROW_D, -7.0), mcia((size_t)B * S, -7.0);
    std::vector<int> res_i((size_t)B * Ps * ZSL_ROW_I, -7), mcia_plane((size_t)B * S, -7), mcia_status((size_t)B * S, -7);
    std::vector<int64_t> res_n((size_t)B * Ps, -7);
    for (size_t t = 0; t < (size_t)B * Ps; ++t) {
        const size_t b = t / (size_t)Ps;
        const int sp = (int)(t - b * (size_t)Ps);
        int flag = ZSL_OK, low = -1, ls = -1;
        double area = zsl_inf(), strain = zsl_inf();
        long long n = 0;
        for (int fp = 0; fp < Pf; ++fp) {
            const size_t item = (b * Pf + fp) * (size_t)Ps + sp;
            flag = zsl_max(flag, clamp_status(item_i[item * ZSL_ROW_I]));
            const double a = item_d[item * ZSL_ROW_D], s = item_d[item * ZSL_ROW_D + 4];
            if (a < area) area = a, low = fp;
            if (s < strain) strain = s, ls = fp;
            n += item_n[item];
        }
        const size_t il = (b * Pf + (low < 0 ? 0 : low)) * (size_t)Ps + sp, is = (b * Pf + (ls < 0 ? 0 : ls)) * (size_t)Ps + sp;
        for (int i = 0; i < 4; ++i) res_d[t * ZSL_ROW_D + i] = item_d[il * ZSL_ROW_D + i];
        for (int i = 4; i < ZSL_ROW_D; ++i) res_d[t * ZSL_ROW_D + i] = item_d[is * ZSL_ROW_D + i];
        for (int i = 1; i < 10; ++i) res_i[t * ZSL_ROW_I + i] = item_i[il * ZSL_ROW_I + i];
        for (int i = 10; i < ZSL_ROW_I; ++i) res_i[t * ZSL_ROW_I + i] = item_i[is * ZSL_ROW_I + i];
        res_i[t * ZSL_ROW_I] = flag != ZSL_OK ? flag : low >= 0 ? ZSL_OK : ZSL_NO_MATCH;
        res_n[t] = count ? n : -1;
    }
    int not_ok = 0;
    for (size_t t = 0; t < (size_t)B * S; ++t) {
        const size_t b = t / (size_t)S;
        const int s = (int)(t - b * (size_t)S);
        int p0 = sub_off[(size_t)s], p1 = sub_off[(size_t)s + 1];
        p0 = p0 < 0 ? 0 : p0, p1 = p1 > Ps ? Ps : p1;
        int flag = ZSL_OK, plane = -1;
        double area = zsl_inf();
        for (int sp = p0; sp < p1; ++sp) {
            const int st = clamp_status(res_i[(b * Ps + sp) * ZSL_ROW_I]);
            flag = zsl_max(flag, st >= ZSL_MULT_CAP ? st : ZSL_OK);
            const double a = res_d[(b * Ps + sp) * ZSL_ROW_D];
            if (a < area) area = a, plane = sp;
        }
        mcia[t] = area, mcia_plane[t] = plane, mcia_status[t] = flag != ZSL_OK ? flag : plane >= 0 ? ZSL_OK : ZSL_NO_MATCH;
        not_ok += mcia_status[t] != ZSL_OK ? 1 : 0;
    }

    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    for (const Planes* p : {&fp_, &sp_}) wr(fo, p->vec), wr(fo, p->area), wr(fo, p->mult), wr(fo, p->status);
    wr(fo, table), wr(fo, res_d), wr(fo, res_i), wr(fo, res_n), wr(fo, mcia), wr(fo, mcia_plane), wr(fo, mcia_status);
    fclose(fo);
    printf("zsl_host_check: %d films x %d substrates, %zu items, %d not OK\n", B, S, items, not_ok);
    return 0;
}
