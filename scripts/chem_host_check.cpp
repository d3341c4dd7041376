// Stand-alone host run of matinvent_amd/csrc/chem_enum.h in the order of the three launches of csrc/chem_valid.hip: the plan
// per crystal, the scan of the chunk counts into the work-item table, the items taken grid-stride by `grid` workgroups of 256 threads with
// one fixed tree per item, the fold per crystal in chunk order.  tests/test_chem_host.py compiles it with -fsanitize=address,undefined and
// compares every output with the restatement (tests/chem_ref.py).
//
//   chem_host_check case.bin out.bin
// case.bin: int32 B, N, use_pauling_test, include_alloys, grid; int64 max_combos; int32 present[119], n_states[119], ox[119][32],
//           eneg_rank[119], is_metal[119], node_off[B + 1], atom_types[N].
// out.bin:  int32 valid[B], status[B], n_elems[B], elems[B][8], counts[B][8]; int64 n_combos[B], n_neutral[B], n_valid[B], first[B];
//           int32 first_ox[B][8], atom_ox[N].  Every output starts at the poison value -77.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../matinvent_amd/csrc/chem_enum.h"

using namespace mi;

template <class T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
    return v;
}

template <class T>
static void wr(FILE* f, const std::vector<T>& v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(3);
}

int main(int argc, char** argv) {
    if (argc != 3) return 64;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 65;
    const std::vector<int> head = rd<int>(f, 5);
    const int B = head[0], N = head[1], use_pauling = head[2], include_alloys = head[3], grid = head[4];
    const int64_t max_combos = rd<int64_t>(f, 1)[0];
    const size_t Z1 = CHEM_MAX_Z + 1;
    const std::vector<int> present = rd<int>(f, Z1), n_states = rd<int>(f, Z1), ox = rd<int>(f, Z1 * CHEM_MAX_STATES), rank = rd<int>(f, Z1), metal = rd<int>(f, Z1);
    const std::vector<int> node_off = rd<int>(f, (size_t)B + 1), types = rd<int>(f, (size_t)N);
    fclose(f);
    if (B < 0 || B > CHEM_MAX_BATCH || N < 0 || grid < 1 || max_combos < 1 || max_combos > CHEM_COMBOS_CAP) return 66;
    const ChemTable T{present.data(), n_states.data(), ox.data(), rank.data(), metal.data()};
    const int POISON = -77;
    std::vector<int> valid(B, POISON), status(B, POISON), n_elems(B, POISON), elems((size_t)B * 8, POISON), counts((size_t)B * 8, POISON), first_ox((size_t)B * 8, POISON),
        atom_ox(N, POISON);
    std::vector<int64_t> n_combos(B, POISON), n_neutral(B, POISON), n_valid(B, POISON), first(B, POISON);

    // launch 1: the plan
    std::vector<ChemPlan> plan(B);
    std::vector<int> chunks(B);
    for (int b = 0; b < B; ++b) {
        const int o0 = node_off[b], o1 = node_off[b + 1];
        const bool range_ok = o0 >= 0 && o0 < o1 && o1 <= N;
        bool bad = !range_ok;
        if (range_ok)
            for (int i = o0; i < o1; ++i) bad = bad || !chem_type_ok(types[i]);
        int cnt[CHEM_MAX_Z + 1] = {0};
        if (!bad)
            for (int z = 1; z <= CHEM_MAX_Z; ++z)
                for (int i = o0; i < o1; ++i) cnt[z] += types[i] == z;
        chem_compose(cnt, bad, T, include_alloys, max_combos, plan[b]);
        chunks[b] = plan[b].n_chunks;
    }

    // launch 2: the scan, then the items grid-stride
    std::vector<int> item_off((size_t)B + 1, 0);
    for (int b = 0; b < B; ++b) item_off[b + 1] = item_off[b] + chunks[b];
    const int n_items = item_off[B];
    std::vector<int64_t> partial((size_t)n_items * 3, POISON);
    for (int wg = 0; wg < grid; ++wg)
        for (int it = wg; it < n_items; it += grid) {
            int lo = 0, hi = B;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (item_off[mid] <= it) lo = mid;
                else hi = mid;
            }
            const int chunk = it - item_off[lo];
            const ChemPlan& p = plan[lo];
            ChemItem item;
            for (int pos = 0; pos < CHEM_MAX_ELEMS; ++pos) {
                chem_item_head(p, pos, item.radix[pos], item.rank[pos]);
                for (int s = 0; s < CHEM_MAX_STATES; ++s) chem_item_cell(p, T, pos, s, item.ox[pos][s], item.w[pos][s]);
            }
            const int64_t c0 = (int64_t)chunk * CHEM_CHUNK;
            int fr[CHEM_THREADS], nn[CHEM_THREADS], nv[CHEM_THREADS];
            for (int tid = 0; tid < CHEM_THREADS; ++tid) {
                const int64_t left = p.n_combos - c0 - (int64_t)tid * CHEM_RUN;
                fr[tid] = CHEM_NO_FIRST, nn[tid] = 0, nv[tid] = 0;
                if (left > 0) {
                    chem_run(item, c0 + (int64_t)tid * CHEM_RUN, left < CHEM_RUN ? (int)left : CHEM_RUN, use_pauling, p.any_unranked, fr[tid], nn[tid], nv[tid]);
                    if (fr[tid] != CHEM_NO_FIRST) fr[tid] += tid * CHEM_RUN;
                }
            }
            for (int w = 0; w < CHEM_THREADS; w += 64)   // the butterfly of a wave leaves its lane 0 with the wave's result
                for (int m = 32; m >= 1; m >>= 1)
                    for (int l = 0; l < m; ++l) {
                        fr[w + l] = fr[w + l + m] < fr[w + l] ? fr[w + l + m] : fr[w + l];
                        nn[w + l] += nn[w + l + m];
                        nv[w + l] += nv[w + l + m];
                    }
            int fmin = fr[0], n1 = nn[0], n2 = nv[0];
            for (int w = 64; w < CHEM_THREADS; w += 64) {
                fmin = fr[w] < fmin ? fr[w] : fmin;
                n1 += nn[w];
                n2 += nv[w];
            }
            partial[(size_t)it * 3 + 0] = fmin == CHEM_NO_FIRST ? -1 : c0 + fmin;
            partial[(size_t)it * 3 + 1] = n1;
            partial[(size_t)it * 3 + 2] = n2;
        }

    // launch 3: the fold and the outputs
    for (int b = 0; b < B; ++b) {
        const ChemPlan& p = plan[b];
        int64_t fst = -1, nn = 0, nv = 0;
        for (int c = 0; c < p.n_chunks; ++c) {
            const int64_t* q = &partial[(size_t)(item_off[b] + c) * 3];
            chem_fold(fst, nn, nv, q[0], q[1], q[2]);
        }
        int fox[CHEM_MAX_ELEMS];
        chem_first_states(p, T, fst, fox);
        for (int e = 0; e < CHEM_MAX_ELEMS; ++e) elems[(size_t)b * 8 + e] = p.elems[e], counts[(size_t)b * 8 + e] = p.counts[e], first_ox[(size_t)b * 8 + e] = fox[e];
        valid[b] = chem_valid(p.status, nv) ? 1 : 0;
        status[b] = p.status, n_elems[b] = p.n_elems, n_combos[b] = p.n_combos, n_neutral[b] = nn, n_valid[b] = nv, first[b] = fst;
        const int o0 = node_off[b], o1 = node_off[b + 1];
        if (!(o0 >= 0 && o0 < o1 && o1 <= N)) continue;
        for (int i = o0; i < o1; ++i) atom_ox[i] = p.status == CHEM_ENUMERATED ? chem_atom_state(p, fox, types[i]) : 0;
    }

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 67;
    wr(o, valid), wr(o, status), wr(o, n_elems), wr(o, elems), wr(o, counts), wr(o, n_combos), wr(o, n_neutral), wr(o, n_valid), wr(o, first), wr(o, first_ox), wr(o, atom_ox);
    fclose(o);
    return 0;
}
