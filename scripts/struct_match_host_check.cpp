// The two kernels of the structure matcher (matinvent_amd/csrc/struct_match.hip) run on the host: the same functions of
// matinvent_amd/csrc/sm_lattice.h and sm_assign.h, in the kernels' order, with the workgroup, wave and lane index as loop variables, the
// ordered compaction written as the serial append it equals, and the lane-per-column assignment (butterfly argmin and shuffles written
// out over 64-entry arrays) checked against the plain-loop sm_assign_serial on every block -- so that the host sanitizers see every
// index the kernels form:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all scripts/struct_match_host_check.cpp -o sm_host_check
//   ./sm_host_check CASE.bin OUT.bin
//
// CASE.bin (little endian): int32 B, N, P; float64 ltol, cos_tol; offsets [B + 1] i32, types [N] i32, frac [N][3] f32, lat [B][9] f32,
// pair_q [P] i32, pair_c [P] i32 (both into the one prepared set).  Every array is a heap block of exactly its size.
// OUT.bin: lat [B][9], inv [B][9], frac [N][3] f64; types [N], perm [N], spec_Z [B][16], spec_off [B][17], info [B][4] i32; then rms [P],
// max_dist [P] f64; best_map [P][9], best_trans [P], n_maps [P], n_items [P], status [P], perm [P][64] i32.  Pre-filled with 0 (-1 for the
// pair outputs' integers, NaN for rms and max_dist).  tests/test_struct_match_host.py writes the cases and compares every output with
// tests/sm_ref64.py bit for bit.  Exit status 3: the lane-per-column assignment and the plain loops disagreed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../matinvent_amd/csrc/sm_assign.h"

using namespace mi;

template <typename T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "sm_host_check: short case file\n");
        exit(2);
    }
    return v;
}
template <typename T>
static void wr(FILE* f, const std::vector<T>& v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

static const int NO_COL = 0x7fffffff;

// sm_wave_assign of struct_match.hip: a lane per column and per row, 64 lanes
static bool wave_assign(const double* tile, int nb, int* col_out) {
    double u[64], v[64], shortest[64];
    int row4col[64], col4row[64], path[64];
    bool SR[64], SC[64];
    for (int l = 0; l < 64; ++l) u[l] = v[l] = 0.0, row4col[l] = col4row[l] = path[l] = -1;
    for (int cur = 0; cur < nb; ++cur) {
        for (int l = 0; l < 64; ++l) shortest[l] = sm_inf(), SR[l] = false, SC[l] = l >= nb;
        double min_val = 0.0;
        int i = cur, sink = -1;
        while (sink < 0) {
            SR[i] = true;
            const double ui = u[i];
            double bv[64];
            int bj[64];
            for (int l = 0; l < 64; ++l) {
                if (!SC[l]) {
                    const double r = sm_reduced(min_val, tile[(size_t)i * nb + l], ui, v[l]);
                    if (r < shortest[l]) shortest[l] = r, path[l] = i;
                }
                bv[l] = SC[l] ? sm_inf() : shortest[l], bj[l] = SC[l] ? NO_COL : l;
            }
            for (int m = 32; m >= 1; m >>= 1) {
                double nv[64];
                int nj[64];
                for (int l = 0; l < 64; ++l) {
                    const int o = l ^ m;
                    const bool take = sm_better(bv[o], bj[o], bv[l], bj[l]);
                    nv[l] = take ? bv[o] : bv[l], nj[l] = take ? bj[o] : bj[l];
                }
                memcpy(bv, nv, sizeof(bv)), memcpy(bj, nj, sizeof(bj));
            }
            if (bj[0] >= nb || !(bv[0] < sm_inf())) return false;
            min_val = bv[0];
            SC[bj[0]] = true;
            const int r4 = row4col[bj[0]];
            if (r4 < 0) sink = bj[0];
            else i = r4;
        }
        double sc[64];
        for (int l = 0; l < 64; ++l) sc[l] = shortest[col4row[l] < 0 ? 0 : col4row[l]];
        for (int l = 0; l < 64; ++l) {
            if (l == cur) u[l] = u[l] + min_val;
            else if (SR[l]) u[l] = u[l] + (min_val - sc[l]);
            if (SC[l] && l < nb) v[l] = v[l] - (min_val - shortest[l]);
        }
        int j = sink;
        for (int step = 0; step <= nb; ++step) {
            const int r = path[j];
            row4col[j] = r;
            const int old = col4row[r];
            col4row[r] = j;
            j = old;
            if (r == cur) break;
        }
    }
    for (int l = 0; l < nb; ++l) col_out[l] = col4row[l];
    return true;
}

struct Prepared {
    std::vector<int> offsets;
    std::vector<double> lat, inv, frac;
    std::vector<int> types, perm, spec_Z, spec_off, info;
    int B, N;
};

struct Pair {
    const double *f1, *f2, *L1, *L2;
    const int *maps, *spec_off;
    int n, nspec, r0, ntrans;
};

static long g_blocks = 0;

// sm_wave_item: exactly sized per-wave arrays
static bool wave_item(const Pair& P, int item, double* rms, double* max_dist, std::vector<int>& col) {
    const int m = item / P.ntrans, j = item - m * P.ntrans;
    int M[9], Mi[9];
    for (int i = 0; i < 9; ++i) M[i] = P.maps[m * 9 + i];
    sm_map_inverse(M, Mi);
    double G[9];
    sm_metric(P.L1, P.L2, M, G);
    std::vector<double> f2p((size_t)P.n * 3), u((size_t)P.n * 3), d2((size_t)P.n);
    col.assign((size_t)P.n, -1);
    for (int lane = 0; lane < P.n; ++lane) sm_map_frac(P.f2 + 3 * lane, Mi, f2p.data() + 3 * lane);
    double t[3];
    for (int c = 0; c < 3; ++c) t[c] = P.f1[3 * (P.r0 + j) + c] - f2p[(size_t)3 * P.r0 + c];
    for (int s = 0; s < P.nspec; ++s) {
        const int b0 = P.spec_off[s], nb = P.spec_off[s + 1] - b0;
        std::vector<double> tile((size_t)nb * nb);
        for (int lane = 0; lane < nb; ++lane)
            for (int a = 0; a < nb; ++a) {
                double uu[3];
                tile[(size_t)a * nb + lane] = sm_pair_cost(G, P.f1 + 3 * (b0 + a), f2p.data() + 3 * (b0 + lane), t, uu);
            }
        std::vector<int> c_lane((size_t)nb), c_serial((size_t)nb);
        SmAssignWork w;
        const bool ok_l = wave_assign(tile.data(), nb, c_lane.data()), ok_s = sm_assign_serial(tile.data(), nb, c_serial.data(), &w);
        if (ok_l != ok_s || (ok_l && c_lane != c_serial)) {
            fprintf(stderr, "sm_host_check: the lane-per-column assignment and the plain loops disagree (block of %d)\n", nb);
            exit(3);
        }
        ++g_blocks;
        if (!ok_l) {
            *rms = sm_inf(), *max_dist = sm_inf();
            return false;
        }
        for (int lane = 0; lane < nb; ++lane) {
            sm_pair_cost(G, P.f1 + 3 * (b0 + lane), f2p.data() + 3 * (b0 + c_lane[(size_t)lane]), t, u.data() + 3 * (b0 + lane));
            col[(size_t)(b0 + lane)] = b0 + c_lane[(size_t)lane];
        }
    }
    double mean[3];
    sm_mean(u.data(), P.n, mean);
    for (int lane = 0; lane < P.n; ++lane) d2[(size_t)lane] = sm_centred(G, u.data() + 3 * lane, mean);
    sm_rms(d2.data(), P.n, rms, max_dist);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: sm_host_check CASE.bin OUT.bin\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const auto head = rd<int>(f, 3);
    const auto tol = rd<double>(f, 2);
    const int B = head[0], N = head[1], NP = head[2];
    const double ltol = tol[0], cos_tol = tol[1];
    Prepared S;
    S.B = B, S.N = N;
    S.offsets = rd<int>(f, (size_t)B + 1);
    const auto types = rd<int>(f, (size_t)N);
    const auto frac = rd<float>(f, (size_t)N * 3), lat = rd<float>(f, (size_t)B * 9);
    const auto pair_q = rd<int>(f, (size_t)NP), pair_c = rd<int>(f, (size_t)NP);
    fclose(f);
    S.lat.assign((size_t)B * 9, 0.0), S.inv.assign((size_t)B * 9, 0.0), S.frac.assign((size_t)N * 3, 0.0);
    S.types.assign((size_t)N, 0), S.perm.assign((size_t)N, 0), S.spec_Z.assign((size_t)B * SM_MAX_SPECIES, 0);
    S.spec_off.assign((size_t)B * (SM_MAX_SPECIES + 1), 0), S.info.assign((size_t)B * 4, 0);
    // ---- sm_prepare_kernel: blockIdx.x = b, threadIdx.x = lane
    for (int b = 0; b < B; ++b) {
        int* info = S.info.data() + (size_t)b * 4;
        const int n0 = S.offsets[(size_t)b], n1 = S.offsets[(size_t)b + 1];
        if (!(n0 >= 0 && n0 <= n1 && n1 <= N)) {
            info[0] = info[1] = info[2] = 0, info[3] = SM_PREP_BAD_INPUT;
            continue;
        }
        const int n = n1 - n0;
        info[0] = n, info[1] = info[2] = 0;
        if (n < 1 || n > SM_MAX_ATOMS) {
            info[3] = n < 1 ? SM_PREP_BAD_INPUT : SM_PREP_TOO_MANY_ATOMS;
            continue;
        }
        const float* L = lat.data() + (size_t)b * 9;
        bool bad = false;
        for (int i = 0; i < 9; ++i) bad = bad || !sm_finite((double)L[i]);
        for (int lane = 0; lane < n; ++lane) {
            const int z = types[(size_t)(n0 + lane)];
            bad = bad || z < 1 || z > SM_MAX_Z;
            for (int c = 0; c < 3; ++c) bad = bad || !sm_finite((double)frac[(size_t)(n0 + lane) * 3 + c]);
        }
        if (bad) {
            info[3] = SM_PREP_BAD_INPUT;
            continue;
        }
        std::vector<int> rank((size_t)n), sidx((size_t)n), cnt((size_t)n);
        std::vector<char> first((size_t)n);
        int nspec = 0;
        for (int lane = 0; lane < n; ++lane) {
            bool fst;
            sm_sort_lane(types.data() + n0, n, lane, &rank[(size_t)lane], &fst, &sidx[(size_t)lane], &cnt[(size_t)lane]);
            first[(size_t)lane] = fst, nspec += fst ? 1 : 0;
        }
        if (nspec > SM_MAX_SPECIES) {
            info[3] = SM_PREP_TOO_MANY_SPECIES;
            continue;
        }
        int T[9];
        double Ls[9], inv[9];
        const int st = sm_prepare_cell(L, n, T, Ls, inv);
        if (st != SM_PREP_OK) {
            info[3] = st;
            continue;
        }
        for (int i = 0; i < 9; ++i) S.lat[(size_t)b * 9 + i] = Ls[i], S.inv[(size_t)b * 9 + i] = inv[i];
        int* so = S.spec_off.data() + (size_t)b * (SM_MAX_SPECIES + 1);
        for (int lane = 0; lane < n; ++lane) {
            const size_t d = (size_t)(n0 + rank[(size_t)lane]);
            sm_reduced_frac(frac.data() + (size_t)(n0 + lane) * 3, T, S.frac.data() + d * 3);
            S.types[d] = types[(size_t)(n0 + lane)], S.perm[d] = lane;
            if (first[(size_t)lane]) S.spec_Z[(size_t)b * SM_MAX_SPECIES + sidx[(size_t)lane]] = types[(size_t)(n0 + lane)], so[sidx[(size_t)lane]] = rank[(size_t)lane];
        }
        for (int lane = nspec; lane <= SM_MAX_SPECIES; ++lane) {
            if (lane < SM_MAX_SPECIES) S.spec_Z[(size_t)b * SM_MAX_SPECIES + lane] = 0;
            so[lane] = n;
        }
        info[1] = nspec, info[2] = sm_rarest(so, nspec), info[3] = SM_PREP_OK;
    }
    // ---- sm_match_kernel: blockIdx.x = p
    const double nan = (double)__builtin_nanf("");
    std::vector<double> rms((size_t)NP, nan), max_dist((size_t)NP, nan);
    std::vector<int> best_map((size_t)NP * 9, -1), best_trans((size_t)NP, -1), n_maps((size_t)NP, -1), n_items((size_t)NP, -1), status((size_t)NP, -1),
        perm((size_t)NP * SM_MAX_ATOMS, -1);
    auto fail = [&](int p, int st, int nm) {
        rms[(size_t)p] = max_dist[(size_t)p] = sm_inf(), best_trans[(size_t)p] = -1, n_maps[(size_t)p] = nm, n_items[(size_t)p] = 0, status[(size_t)p] = st;
        for (int i = 0; i < 9; ++i) best_map[(size_t)p * 9 + i] = 0;
        for (int i = 0; i < SM_MAX_ATOMS; ++i) perm[(size_t)p * SM_MAX_ATOMS + i] = -1;
    };
    long items_n = 0;
    for (int p = 0; p < NP; ++p) {
        const int q = pair_q[(size_t)p], c = pair_c[(size_t)p];
        if (q < 0 || q >= B || c < 0 || c >= B) {
            fail(p, SM_BAD_PAIR, 0);
            continue;
        }
        const int *ia = S.info.data() + (size_t)q * 4, *ib = S.info.data() + (size_t)c * 4;
        if (ia[3] != SM_PREP_OK || ib[3] != SM_PREP_OK) {
            fail(p, SM_NOT_PREPARED, 0);
            continue;
        }
        const int n = ia[0];
        const int *oa = S.spec_off.data() + (size_t)q * (SM_MAX_SPECIES + 1), *ob = S.spec_off.data() + (size_t)c * (SM_MAX_SPECIES + 1);
        bool same = ia[0] == ib[0] && ia[1] == ib[1];
        for (int s = 0; s < SM_MAX_SPECIES; ++s)
            same = same && S.spec_Z[(size_t)q * SM_MAX_SPECIES + s] == S.spec_Z[(size_t)c * SM_MAX_SPECIES + s] && oa[s] == ob[s];
        if (!same) {
            fail(p, SM_SPECIES_MISMATCH, 0);
            continue;
        }
        const double *L1 = S.lat.data() + (size_t)q * 9, *L2 = S.lat.data() + (size_t)c * 9;
        SmTarget tg;
        sm_target(L1, &tg);
        int bound[3];
        const int pts = sm_box(tg, S.inv.data() + (size_t)c * 9, ltol, bound);
        if (pts < 0) {
            fail(p, SM_BOX_CAP_HIT, 0);
            continue;
        }
        std::vector<double> cand_v((size_t)3 * SM_MAX_CAND * 3), cand_len((size_t)3 * SM_MAX_CAND);
        std::vector<int> cand_k((size_t)3 * SM_MAX_CAND * 3);
        int ncand[3] = {0, 0, 0};
        for (int pt = 0; pt < pts; ++pt) {   // (the ordered compaction of a round of 256 points is the serial append)
            int k[3];
            double v[3], len;
            sm_box_point(pt, bound, L2, k, v, &len);
            for (int ax = 0; ax < 3; ++ax)
                if (sm_length_ok(len, tg.len[ax], ltol)) {
                    if (ncand[ax] < SM_MAX_CAND) {
                        const size_t e = (size_t)ax * SM_MAX_CAND + (size_t)ncand[ax];
                        for (int i = 0; i < 3; ++i) cand_v[3 * e + i] = v[i], cand_k[3 * e + i] = k[i];
                        cand_len[e] = len;
                    }
                    ++ncand[ax];
                }
        }
        if (ncand[0] > SM_MAX_CAND || ncand[1] > SM_MAX_CAND || ncand[2] > SM_MAX_CAND) {
            fail(p, SM_BOX_CAP_HIT, 0);
            continue;
        }
        std::vector<int> maps((size_t)SM_MAX_MAPS * 9);
        const int64_t triples = (int64_t)ncand[0] * ncand[1] * ncand[2];
        int nmaps = 0;
        for (int64_t t = 0; t < triples && nmaps <= SM_MAX_MAPS; ++t) {
            const size_t e0 = (size_t)(t / ((int64_t)ncand[1] * ncand[2])), e1 = (size_t)SM_MAX_CAND + (size_t)((t / ncand[2]) % ncand[1]),
                         e2 = (size_t)2 * SM_MAX_CAND + (size_t)(t % ncand[2]);
            if (!sm_triple_ok(tg, &cand_v[3 * e0], cand_len[e0], &cand_k[3 * e0], &cand_v[3 * e1], cand_len[e1], &cand_k[3 * e1], &cand_v[3 * e2], cand_len[e2],
                              &cand_k[3 * e2], cos_tol))
                continue;
            if (nmaps < SM_MAX_MAPS)
                for (int i = 0; i < 3; ++i)
                    maps[(size_t)nmaps * 9 + i] = cand_k[3 * e0 + i], maps[(size_t)nmaps * 9 + 3 + i] = cand_k[3 * e1 + i], maps[(size_t)nmaps * 9 + 6 + i] = cand_k[3 * e2 + i];
            ++nmaps;
        }
        if (nmaps > SM_MAX_MAPS || nmaps == 0) {
            fail(p, nmaps == 0 ? SM_NO_LATTICE : SM_MAP_CAP_HIT, nmaps > SM_MAX_MAPS ? SM_MAX_MAPS : 0);
            continue;
        }
        const int rarest = ib[2], n0a = S.offsets[(size_t)q], n0b = S.offsets[(size_t)c];
        const Pair P{S.frac.data() + (size_t)n0a * 3, S.frac.data() + (size_t)n0b * 3, L1, L2, maps.data(), oa, n, ia[1], oa[rarest], oa[rarest + 1] - oa[rarest]};
        const int items = nmaps * P.ntrans;
        double wb[4], wm[4];
        int wi[4];
        std::vector<int> col;
        for (int wave = 0; wave < 4; ++wave) {
            wb[wave] = wm[wave] = sm_inf(), wi[wave] = NO_COL;
            for (int item = wave; item < items; item += 4) {
                double r, md;
                wave_item(P, item, &r, &md, col);
                ++items_n;
                if (sm_better(r, item, wb[wave], wi[wave])) wb[wave] = r, wm[wave] = md, wi[wave] = item;
            }
        }
        double best = wb[0], best_m = wm[0];
        int best_i = wi[0];
        for (int w = 1; w < 4; ++w)
            if (sm_better(wb[w], wi[w], best, best_i)) best = wb[w], best_m = wm[w], best_i = wi[w];
        const bool found = best_i != NO_COL;
        rms[(size_t)p] = found ? best : sm_inf(), max_dist[(size_t)p] = found ? best_m : sm_inf();
        best_trans[(size_t)p] = found ? best_i % P.ntrans : -1, n_maps[(size_t)p] = nmaps, n_items[(size_t)p] = items, status[(size_t)p] = SM_OK;
        for (int i = 0; i < 9; ++i) best_map[(size_t)p * 9 + i] = found ? maps[(size_t)(best_i / P.ntrans) * 9 + i] : 0;
        double r, md;
        const bool ok = found && wave_item(P, best_i, &r, &md, col);
        for (int lane = 0; lane < SM_MAX_ATOMS; ++lane) perm[(size_t)p * SM_MAX_ATOMS + lane] = -1;
        if (ok)
            for (int lane = 0; lane < n; ++lane) perm[(size_t)p * SM_MAX_ATOMS + S.perm[(size_t)(n0a + lane)]] = S.perm[(size_t)(n0b + col[(size_t)lane])];
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    wr(o, S.lat), wr(o, S.inv), wr(o, S.frac), wr(o, S.types), wr(o, S.perm), wr(o, S.spec_Z), wr(o, S.spec_off), wr(o, S.info);
    wr(o, rms), wr(o, max_dist), wr(o, best_map), wr(o, best_trans), wr(o, n_maps), wr(o, n_items), wr(o, status), wr(o, perm);
    fclose(o);
    printf("sm_host_check: %d crystals, %d pairs, %ld items, %ld blocks assigned twice and equal\n", B, NP, items_n, g_blocks);
    return 0;
}
