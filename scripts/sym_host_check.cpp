// The kernels of the symmetry finder (matinvent_amd/csrc/symmetry.hip) run on the host: the same functions of matinvent_amd/csrc/sym_ops.h,
// sm_lattice.h and sm_assign.h, in the kernels' order, with the workgroup, wave and lane index as loop variables, the ordered compactions
// written as the serial appends they equal, the rounds of four items folded in item order, and the bijection through one slot per target
// checked against a plain seen-array loop on every item -- so that the host sanitizers see every index the kernels form:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all scripts/sym_host_check.cpp -o sym_host_check
//   ./sym_host_check CASE.bin OUT.bin
//
// CASE.bin (little endian): int32 B, N; float64 cos_tol; offsets [B + 1] i32, types [N] i32, frac [N][3] f32, lat [B][9] f32, tol [B] f64.
// Every array is a heap block of exactly its size.
// OUT.bin: info [B][8], rot_hist [B][10], rot [B][192][9] i32; trans [B][192][3], dev [B][192], ptrans [B][64][3] f64; prim_count [B],
// prim_status [B] i32; prim_det [B] f64; prim_offsets [B + 1], types [N] i32; frac [N][3], lat [B][9] f32.  Pre-filled with -7.
// tests/test_symmetry_host.py writes the cases and compares every output with tests/sym_ref64.py bit for bit.  Exit status 3: the slot
// bijection and the plain loop disagreed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../matinvent_amd/csrc/sym_ops.h"

using namespace mi;

template <typename T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "sym_host_check: short case file\n");
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
        fprintf(stderr, "usage: sym_host_check CASE.bin OUT.bin\n");
        return 2;
    }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    const auto head = rd<int>(fi, 2);
    const double cos_tol = rd<double>(fi, 1)[0];
    const int B = head[0], N = head[1];
    const auto offsets = rd<int>(fi, (size_t)B + 1);
    const auto types = rd<int>(fi, (size_t)N);
    const auto frac = rd<float>(fi, (size_t)N * 3), lat = rd<float>(fi, (size_t)B * 9);
    const auto tols = rd<double>(fi, (size_t)B);
    fclose(fi);
    // ---- sm_prepare_kernel (struct_match.hip), as scripts/struct_match_host_check.cpp runs it
    std::vector<double> p_lat((size_t)B * 9, 0.0), p_inv((size_t)B * 9, 0.0), p_frac((size_t)N * 3, 0.0);
    std::vector<int> p_types((size_t)N, 0), p_perm((size_t)N, 0), p_spec_off((size_t)B * (SM_MAX_SPECIES + 1), 0), p_info((size_t)B * 4, 0);
    for (int b = 0; b < B; ++b) {
        int* info = p_info.data() + (size_t)b * 4;
        const int n0 = offsets[(size_t)b], n1 = offsets[(size_t)b + 1];
        info[3] = SM_PREP_BAD_INPUT;
        if (!(n0 >= 0 && n0 <= n1 && n1 <= N)) continue;
        const int n = n1 - n0;
        info[0] = n;
        if (n < 1) continue;
        if (n > SM_MAX_ATOMS) {
            info[3] = SM_PREP_TOO_MANY_ATOMS;
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
        if (bad) continue;
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
        for (int i = 0; i < 9; ++i) p_lat[(size_t)b * 9 + i] = Ls[i], p_inv[(size_t)b * 9 + i] = inv[i];
        int* so = p_spec_off.data() + (size_t)b * (SM_MAX_SPECIES + 1);
        for (int lane = 0; lane < n; ++lane) {
            const size_t d = (size_t)(n0 + rank[(size_t)lane]);
            sm_reduced_frac(frac.data() + (size_t)(n0 + lane) * 3, T, p_frac.data() + d * 3);
            p_types[d] = types[(size_t)(n0 + lane)], p_perm[d] = lane;
            if (first[(size_t)lane]) so[sidx[(size_t)lane]] = rank[(size_t)lane];
        }
        for (int lane = nspec; lane <= SM_MAX_SPECIES; ++lane) so[lane] = n;
        info[1] = nspec, info[2] = sm_rarest(so, nspec), info[3] = SM_PREP_OK;
    }
    // ---- sym_find_kernel: blockIdx.x = b
    const int POISON = -7;
    std::vector<int> o_info((size_t)B * SYM_INFO, POISON), o_hist((size_t)B * SYM_CLASSES, POISON), o_rot((size_t)B * SYM_MAX_OPS * 9, POISON);
    std::vector<double> o_trans((size_t)B * SYM_MAX_OPS * 3, (double)POISON), o_dev((size_t)B * SYM_MAX_OPS, (double)POISON),
        o_ptrans((size_t)B * SYM_MAX_TRANS * 3, (double)POISON);
    auto fail = [&](int b, int st) {
        for (int i = 0; i < SYM_INFO; ++i) o_info[(size_t)b * SYM_INFO + i] = i == SYM_INFO - 1 ? st : 0;
        for (int i = 0; i < SYM_CLASSES; ++i) o_hist[(size_t)b * SYM_CLASSES + i] = 0;
    };
    long items_n = 0;
    for (int b = 0; b < B; ++b) {
        const int* pinfo = p_info.data() + (size_t)b * 4;
        if (pinfo[3] != SM_PREP_OK) {
            fail(b, SYM_NOT_PREPARED);
            continue;
        }
        const double tol = tols[(size_t)b];
        if (!sym_tol_ok(tol)) {
            fail(b, SYM_BAD_TOL);
            continue;
        }
        const int n = pinfo[0], nspec = pinfo[1], rarest = pinfo[2], n0 = offsets[(size_t)b];
        const int* spec_off = p_spec_off.data() + (size_t)b * (SM_MAX_SPECIES + 1);
        const double* L = p_lat.data() + (size_t)b * 9;
        std::vector<double> f(p_frac.begin() + (size_t)n0 * 3, p_frac.begin() + (size_t)(n0 + n) * 3);
        std::vector<int> blk0((size_t)n), blkn((size_t)n);
        for (int tid = 0; tid < n; ++tid) {
            int s = 0;
            for (int e = 1; e < nspec; ++e) s += spec_off[e] <= tid ? 1 : 0;
            blk0[(size_t)tid] = spec_off[s], blkn[(size_t)tid] = spec_off[s + 1] - spec_off[s];
        }
        SmTarget tg;
        sm_target(L, &tg);
        int bound[3];
        const int pts = sym_box(tg, p_inv.data() + (size_t)b * 9, tol, bound);
        if (pts < 0) {
            fail(b, SYM_BOX_CAP);
            continue;
        }
        std::vector<double> cand_v((size_t)3 * SM_MAX_CAND * 3), cand_len((size_t)3 * SM_MAX_CAND);
        std::vector<int> cand_k((size_t)3 * SM_MAX_CAND * 3);
        int ncand[3] = {0, 0, 0};
        for (int pt = 0; pt < pts; ++pt) {
            int k[3];
            double v[3], len;
            sm_box_point(pt, bound, L, k, v, &len);
            for (int ax = 0; ax < 3; ++ax)
                if (sym_length_ok(len, tg.len[ax], tol)) {
                    if (ncand[ax] < SM_MAX_CAND) {
                        const size_t e = (size_t)ax * SM_MAX_CAND + (size_t)ncand[ax];
                        for (int i = 0; i < 3; ++i) cand_v[3 * e + i] = v[i], cand_k[3 * e + i] = k[i];
                        cand_len[e] = len;
                    }
                    ++ncand[ax];
                }
        }
        if (ncand[0] > SM_MAX_CAND || ncand[1] > SM_MAX_CAND || ncand[2] > SM_MAX_CAND) {
            fail(b, SYM_BOX_CAP);
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
            fail(b, nmaps == 0 ? SYM_NO_LATTICE : SYM_MAP_CAP);
            continue;
        }
        const int r0 = spec_off[rarest], ntrans = spec_off[rarest + 1] - spec_off[rarest];
        const int items = nmaps * ntrans;
        double G[9];
        sym_metric(L, G);
        int n_ops = 0, n_trans = 0, pg_order = 0, last_map = -1, status = SYM_OK;
        int hist[SYM_CLASSES] = {0};
        for (int base = 0; base < items; base += 4) {
            int acc[4] = {0, 0, 0, 0};
            double w_dev[4], w_t[4][3];
            std::vector<double> w_u[4];
            for (int wave = 0; wave < 4; ++wave) {
                const int item = base + wave;
                if (item >= items) continue;
                ++items_n;
                const int m = item / ntrans, j = item - m * ntrans;
                int Mi[9];
                sm_map_inverse(maps.data() + (size_t)m * 9, Mi);
                std::vector<double> fp((size_t)n * 3), u((size_t)n * 3);
                std::vector<int> tgt((size_t)n), hit((size_t)n, -1);   // exactly sized: a target outside the crystal is an error here
                for (int lane = 0; lane < n; ++lane) sm_map_frac(f.data() + 3 * lane, Mi, fp.data() + 3 * lane);
                double t[3];
                for (int c = 0; c < 3; ++c) t[c] = f[(size_t)3 * (r0 + j) + c] - fp[(size_t)3 * r0 + c];
                bool within = true;
                double dev = 0.0;
                for (int lane = 0; lane < n; ++lane) {
                    double d2;
                    tgt[(size_t)lane] = sym_nearest(G, f.data(), blk0[(size_t)lane], blkn[(size_t)lane], fp.data() + 3 * lane, t, u.data() + 3 * lane, &d2) ;
                    const double d = sqrt(d2);
                    within = within && d <= tol;
                    dev = d > dev ? d : dev;
                    hit[(size_t)tgt[(size_t)lane]] = lane;
                }
                bool bij = true;
                for (int lane = 0; lane < n; ++lane) bij = bij && hit[(size_t)tgt[(size_t)lane]] == lane;
                std::vector<char> seen((size_t)n, 0);   // the plain loop
                bool plain = true;
                for (int lane = 0; lane < n; ++lane) {
                    plain = plain && !seen[(size_t)tgt[(size_t)lane]];
                    seen[(size_t)tgt[(size_t)lane]] = 1;
                }
                if (plain != bij) {
                    fprintf(stderr, "sym_host_check: the slot bijection and the plain loop disagree (crystal %d, item %d)\n", b, item);
                    return 3;
                }
                acc[wave] = ((within && bij) ? 1 : 0) | ((within && !bij) ? 2 : 0);
                w_dev[wave] = dev, w_t[wave][0] = t[0], w_t[wave][1] = t[1], w_t[wave][2] = t[2];
                w_u[wave] = u;
            }
            for (int w = 0; w < 4; ++w) {
                const int it = base + w;
                if (it >= items) continue;
                if (acc[w] & 2) status |= SYM_AMBIGUOUS;
                if (!(acc[w] & 1)) continue;
                const int m = it / ntrans;
                const int* Mw = maps.data() + (size_t)m * 9;
                if (m != last_map) {
                    last_map = m, ++pg_order;
                    const int cls = sym_class(Mw);
                    if (cls < 0) status |= SYM_NOT_A_GROUP;
                    else ++hist[cls];
                }
                if (n_ops < SYM_MAX_OPS) {
                    const size_t e = (size_t)b * SYM_MAX_OPS + (size_t)n_ops;
                    for (int i = 0; i < 9; ++i) o_rot[e * 9 + i] = Mw[i];
                    for (int c = 0; c < 3; ++c) o_trans[e * 3 + c] = sm_wrap01(w_t[w][c]);
                    o_dev[e] = w_dev[w];
                }
                if (sym_is_identity(Mw)) {
                    double mean[3];
                    sm_mean(w_u[w].data(), n, mean);
                    for (int c = 0; c < 3; ++c) o_ptrans[((size_t)b * SYM_MAX_TRANS + (size_t)n_trans) * 3 + c] = sm_wrap01(w_t[w][c] - mean[c]);
                    ++n_trans;
                }
                ++n_ops;
            }
        }
        if (n_ops > SYM_MAX_OPS) status |= SYM_OPS_CAP;
        if (n_ops != pg_order * n_trans) status |= SYM_NOT_A_GROUP;
        const int pg = sym_point_group(hist);
        if (pg == 0) status |= SYM_NOT_A_GROUP;
        int* oi = o_info.data() + (size_t)b * SYM_INFO;
        oi[0] = n_ops, oi[1] = n_trans, oi[2] = nmaps, oi[3] = pg_order, oi[4] = pg, oi[5] = sym_crystal_system(pg), oi[6] = hist[4] > 0 ? 1 : 0, oi[7] = status;
        for (int c = 0; c < SYM_CLASSES; ++c) o_hist[(size_t)b * SYM_CLASSES + c] = hist[c];
    }
    // ---- sym_prim_kernel: blockIdx.x = b
    std::vector<int> ws_types((size_t)N, POISON), prim_count((size_t)B, POISON), prim_status((size_t)B, POISON), prim_off((size_t)B + 1, POISON), out_types((size_t)N, POISON);
    std::vector<float> ws_frac((size_t)N * 3, (float)POISON), out_frac((size_t)N * 3, (float)POISON), out_lat((size_t)B * 9, (float)POISON);
    std::vector<double> prim_det((size_t)B, (double)POISON);
    auto copy = [&](int b, int n0, int n, int st) {
        for (int i = 0; i < n; ++i) {
            ws_types[(size_t)(n0 + i)] = types[(size_t)(n0 + i)];
            for (int c = 0; c < 3; ++c) ws_frac[(size_t)(n0 + i) * 3 + c] = frac[(size_t)(n0 + i) * 3 + c];
        }
        for (int i = 0; i < 9; ++i) out_lat[(size_t)b * 9 + i] = lat[(size_t)b * 9 + i];
        prim_count[(size_t)b] = n, prim_status[(size_t)b] = st, prim_det[(size_t)b] = 1.0;
    };
    for (int b = 0; b < B; ++b) {
        const int n0 = offsets[(size_t)b], n1 = offsets[(size_t)b + 1];
        const int sym_status = o_info[(size_t)b * SYM_INFO + SYM_INFO - 1], ntr = o_info[(size_t)b * SYM_INFO + 1];
        if (!(n0 >= 0 && n0 <= n1 && n1 <= N)) {
            copy(b, 0, 0, sym_status);
            continue;
        }
        const int n = n1 - n0;
        if ((sym_status & ~SYM_OPS_CAP) != SYM_OK || ntr <= 1 || ntr > SYM_MAX_TRANS || n > SM_MAX_ATOMS) {
            copy(b, n0, n, sym_status);
            continue;
        }
        std::vector<double> f(p_frac.begin() + (size_t)n0 * 3, p_frac.begin() + (size_t)(n0 + n) * 3);
        std::vector<double> pt(o_ptrans.begin() + (size_t)b * SYM_MAX_TRANS * 3, o_ptrans.begin() + ((size_t)b * SYM_MAX_TRANS + (size_t)ntr) * 3);
        const int m = ntr + 3;
        int bi = -1, bj = -1, bk = -1;
        for (int i = 0; i < m - 2 && bi < 0; ++i)
            for (int j = i + 1; j < m - 1 && bi < 0; ++j)
                for (int k = j + 1; k < m && bi < 0; ++k) {   // (the lowest set lane of the ballot is the first k)
                    double P[9];
                    if (sym_prim_det_ok(sym_prim_det(pt.data(), ntr, i, j, k, P), ntr)) bi = i, bj = j, bk = k;
                }
        if (bi < 0) {
            copy(b, n0, n, sym_status | SYM_PRIM_FAIL);
            continue;
        }
        double P[9], Pinv[9];
        const double det = sym_prim_det(pt.data(), ntr, bi, bj, bk, P);
        sm_inv3(P, det, Pinv);
        const int* spec_off = p_spec_off.data() + (size_t)b * (SM_MAX_SPECIES + 1);
        const int nspec = p_info[(size_t)b * 4 + 1];
        double G[9];
        sym_metric(p_lat.data() + (size_t)b * 9, G);
        std::vector<int> keep_c((size_t)n, 0), src((size_t)n, 0);
        int kept = 0;
        for (int lane = 0; lane < n; ++lane) {
            int s = 0;
            for (int e = 1; e < nspec; ++e) s += spec_off[e] <= lane ? 1 : 0;
            const int b0 = spec_off[s], nb = spec_off[s + 1] - b0;
            bool keep = true;
            for (int p = 1; p < ntr; ++p) {
                double u[3], d2;
                keep = keep && sym_nearest(G, f.data(), b0, nb, f.data() + 3 * lane, pt.data() + 3 * p, u, &d2) > lane;
            }
            const int c = p_perm[(size_t)(n0 + lane)];
            keep_c[(size_t)c] = keep ? 1 : 0, src[(size_t)c] = lane, kept += keep ? 1 : 0;
        }
        if (kept * ntr != n) {
            copy(b, n0, n, sym_status | SYM_PRIM_FAIL);
            continue;
        }
        int at = n0;
        for (int lane = 0; lane < n; ++lane)
            if (keep_c[(size_t)lane]) {
                sym_prim_frac(f.data() + 3 * src[(size_t)lane], Pinv, ws_frac.data() + (size_t)at * 3);
                ws_types[(size_t)at] = types[(size_t)(n0 + lane)];
                ++at;
            }
        int T[9];
        double L0[9], Lr[9];
        for (int i = 0; i < 9; ++i) L0[i] = (double)lat[(size_t)b * 9 + i];
        sm_reduce(L0, T, Lr);
        for (int i = 0; i < 3; ++i) {
            double row[3];
            sym_prim_row(P, Lr, i, row);
            for (int c = 0; c < 3; ++c) out_lat[(size_t)b * 9 + 3 * i + c] = (float)row[c];
        }
        prim_count[(size_t)b] = kept, prim_status[(size_t)b] = sym_status, prim_det[(size_t)b] = sm_abs(det);
    }
    // ---- sym_scan_kernel and sym_gather_kernel
    prim_off[0] = 0;
    for (int b = 0; b < B; ++b) prim_off[(size_t)b + 1] = prim_off[(size_t)b] + prim_count[(size_t)b];
    for (int b = 0; b < B; ++b) {
        const int cnt = prim_count[(size_t)b], dst = prim_off[(size_t)b];
        if (cnt <= 0) continue;
        const int n0 = offsets[(size_t)b];
        for (int i = 0; i < cnt && dst + i < N; ++i) {
            out_types[(size_t)(dst + i)] = ws_types[(size_t)(n0 + i)];
            for (int c = 0; c < 3; ++c) out_frac[(size_t)(dst + i) * 3 + c] = ws_frac[(size_t)(n0 + i) * 3 + c];
        }
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    wr(o, o_info), wr(o, o_hist), wr(o, o_rot), wr(o, o_trans), wr(o, o_dev), wr(o, o_ptrans);
    wr(o, prim_count), wr(o, prim_status), wr(o, prim_det), wr(o, prim_off), wr(o, out_types), wr(o, out_frac), wr(o, out_lat);
    fclose(o);
    printf("sym_host_check: %d crystals, %ld items, every bijection decided twice and equal\n", B, items_n);
    return 0;
}
