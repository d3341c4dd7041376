// Composition validity (include/matinvent_hip_chem.h): every piece of arithmetic of the three launches, host and device, integers
// only.  csrc/chem_valid.hip runs these functions on the device; scripts/chem_host_check.cpp runs them in the kernels' order on the host.
//   chem_compose   one lane: the composition from the per-Z atom counts, the gcd, the status in the header's order, N and the chunk count
//   chem_item_cell one cell of an item's state table, RIGHT-aligned over 8 positions (position 7 is the last element, the fastest digit;
//                  the positions before the first element have radix 1 and the state 0, so the odometer's carry runs through them)
//   chem_run       one thread's contiguous run of a chunk: the first index decoded once by division, then the odometer with the charge sum
//                  carried incrementally; the Pauling test only at a neutral combination
//   chem_fold      one item's partials into a crystal's totals, in chunk order
//   chem_finish    a crystal's scalar outputs and the states of `first`
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CHEM_HD __host__ __device__ __forceinline__
#else
#define CHEM_HD inline
#endif

namespace mi {

constexpr int CHEM_MAX_Z = 118, CHEM_MAX_STATES = 32, CHEM_MAX_ELEMS = 8, CHEM_CHUNK = 65536, CHEM_THREADS = 256, CHEM_MAX_GRID = 2048, CHEM_MAX_BATCH = 4096;
constexpr int CHEM_RUN = CHEM_CHUNK / CHEM_THREADS;   // combinations per thread and item
constexpr int64_t CHEM_COMBOS_CAP = (int64_t)1 << 40; // 32^8: the largest N that 8 lists of 32 can give
constexpr int CHEM_NO_FIRST = 0x7fffffff;
enum : int { CHEM_ENUMERATED = 0, CHEM_ELEMENTAL = 1, CHEM_ALLOY = 2, CHEM_BAD_INPUT = 3, CHEM_TOO_MANY_ELEMENTS = 4, CHEM_UNKNOWN_ELEMENT = 5, CHEM_NO_STATES = 6,
              CHEM_TOO_MANY_COMBOS = 7 };

struct ChemTable {
    const int* present;    // [119]
    const int* n_states;   // [119]
    const int* ox;         // [119][32]
    const int* rank;       // [119]
    const int* metal;      // [119]
};

struct ChemPlan {
    int status, n_elems, any_unranked, n_chunks;
    int elems[CHEM_MAX_ELEMS], counts[CHEM_MAX_ELEMS], radix[CHEM_MAX_ELEMS], rank[CHEM_MAX_ELEMS];   // left-aligned, ascending Z
    int64_t n_combos;
};

// An item's state table in the right-aligned form.
struct ChemItem {
    int radix[CHEM_MAX_ELEMS], rank[CHEM_MAX_ELEMS];
    int ox[CHEM_MAX_ELEMS][CHEM_MAX_STATES];
    int64_t w[CHEM_MAX_ELEMS][CHEM_MAX_STATES];   // ox x count
};

CHEM_HD bool chem_type_ok(int z) { return z >= 1 && z <= CHEM_MAX_Z; }

CHEM_HD int chem_gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b, b = t;
    }
    return a;
}

CHEM_HD bool chem_row_present(const ChemTable& T, int z) { return T.present[z] != 0 && T.n_states[z] >= 0 && T.n_states[z] <= CHEM_MAX_STATES; }

// cnt[z], z = 1 .. 118: the crystal's atoms of type z (not read when `bad`).  `bad`: zero atoms, a type outside 1 .. 118 or bad offsets.
CHEM_HD void chem_compose(const int* cnt, bool bad, const ChemTable& T, int include_alloys, int64_t max_combos, ChemPlan& p) {
    p.status = CHEM_BAD_INPUT, p.n_elems = 0, p.any_unranked = 0, p.n_chunks = 0, p.n_combos = 0;
    for (int e = 0; e < CHEM_MAX_ELEMS; ++e) p.elems[e] = 0, p.counts[e] = 0, p.radix[e] = 1, p.rank[e] = -1;
    if (bad) return;
    int E = 0, g = 0;
    for (int z = 1; z <= CHEM_MAX_Z; ++z) {
        if (cnt[z] <= 0) continue;
        if (E < CHEM_MAX_ELEMS) p.elems[E] = z, p.counts[E] = cnt[z];
        g = chem_gcd(g, cnt[z]);
        ++E;
    }
    if (E == 0) return;   // (zero atoms arrives as `bad`; kept for a caller that did not say so)
    p.n_elems = E;
    const int kept = E < CHEM_MAX_ELEMS ? E : CHEM_MAX_ELEMS;
    for (int e = 0; e < kept; ++e) p.counts[e] /= g;
    if (E == 1) {
        p.status = CHEM_ELEMENTAL;
        return;
    }
    if (E > CHEM_MAX_ELEMS) {
        p.status = CHEM_TOO_MANY_ELEMENTS;
        return;
    }
    bool known = true, metals = true, empty = false;
    for (int e = 0; e < E; ++e) known = known && chem_row_present(T, p.elems[e]);
    if (!known) {
        p.status = CHEM_UNKNOWN_ELEMENT;
        return;
    }
    int64_t N = 1;
    for (int e = 0; e < E; ++e) {
        const int z = p.elems[e];
        metals = metals && T.metal[z] != 0;
        p.radix[e] = T.n_states[z];
        p.rank[e] = T.rank[z];
        if (T.rank[z] < 0) p.any_unranked = 1;
        if (T.n_states[z] == 0) empty = true;
        N *= (int64_t)T.n_states[z];   // at most 32^8 = 2^40
    }
    if (include_alloys && metals) {
        p.status = CHEM_ALLOY;
        return;
    }
    p.n_combos = N;
    if (empty) {
        p.status = CHEM_NO_STATES;
        return;
    }
    if (N > max_combos) {
        p.status = CHEM_TOO_MANY_COMBOS;
        return;
    }
    p.status = CHEM_ENUMERATED;
    p.n_chunks = (int)((N + CHEM_CHUNK - 1) / CHEM_CHUNK);
}

// Cell (pos, s) of the right-aligned table: element e = pos - (8 - E), or padding before it.
CHEM_HD void chem_item_cell(const ChemPlan& p, const ChemTable& T, int pos, int s, int& ox, int64_t& w) {
    const int e = pos - (CHEM_MAX_ELEMS - p.n_elems);
    ox = 0, w = 0;
    if (e >= 0 && s < p.radix[e]) {
        ox = T.ox[p.elems[e] * CHEM_MAX_STATES + s];
        w = (int64_t)ox * (int64_t)p.counts[e];
    }
}
CHEM_HD void chem_item_head(const ChemPlan& p, int pos, int& radix, int& rank) {
    const int e = pos - (CHEM_MAX_ELEMS - p.n_elems);
    radix = e >= 0 ? p.radix[e] : 1;
    rank = e >= 0 ? p.rank[e] : -1;
}

// Combinations start .. start + len - 1 of the item (len >= 1).  first_rel: the lowest passing index minus `start`, or CHEM_NO_FIRST.
CHEM_HD void chem_run(const ChemItem& it, int64_t start, int len, int use_pauling, int any_unranked, int& first_rel, int& n_neutral, int& n_valid) {
    int radix[CHEM_MAX_ELEMS], d[CHEM_MAX_ELEMS];
    int64_t idx = start, sum = 0;
#pragma unroll
    for (int p = CHEM_MAX_ELEMS - 1; p >= 0; --p) {
        radix[p] = it.radix[p];
        d[p] = (int)(idx % radix[p]);
        idx /= radix[p];
        sum += it.w[p][d[p]];
    }
    first_rel = CHEM_NO_FIRST, n_neutral = 0, n_valid = 0;
    for (int i = 0; i < len; ++i) {
        if (sum == 0) {
            ++n_neutral;
            bool pass = true;
            if (use_pauling) {
                int max_pos = -1, min_neg = 0x7fffffff;
#pragma unroll
                for (int p = 0; p < CHEM_MAX_ELEMS; ++p) {
                    const int o = it.ox[p][d[p]], r = it.rank[p];
                    if (o > 0 && r > max_pos) max_pos = r;
                    if (o < 0 && r < min_neg) min_neg = r;
                }
                pass = !any_unranked && max_pos < min_neg;
            }
            if (pass) {
                ++n_valid;
                if (first_rel == CHEM_NO_FIRST) first_rel = i;
            }
        }
        bool carry = true;   // the odometer: position 7 steps every time
#pragma unroll
        for (int p = CHEM_MAX_ELEMS - 1; p >= 0; --p) {
            if (carry) {
                const int od = d[p];
                int nd = od + 1;
                if (nd == radix[p]) nd = 0;
                else carry = false;
                sum += it.w[p][nd] - it.w[p][od];
                d[p] = nd;
            }
        }
    }
}

CHEM_HD void chem_fold(int64_t& first, int64_t& n_neutral, int64_t& n_valid, int64_t item_first, int64_t item_neutral, int64_t item_valid) {
    if (item_first >= 0 && (first < 0 || item_first < first)) first = item_first;
    n_neutral += item_neutral;
    n_valid += item_valid;
}

CHEM_HD bool chem_valid(int status, int64_t n_valid) {
    return status == CHEM_ELEMENTAL || status == CHEM_ALLOY || (status == CHEM_ENUMERATED && n_valid > 0);
}

// The states of combination `first` (left-aligned; 0 past E or when first < 0).
CHEM_HD void chem_first_states(const ChemPlan& p, const ChemTable& T, int64_t first, int* first_ox) {
    for (int e = 0; e < CHEM_MAX_ELEMS; ++e) first_ox[e] = 0;
    if (p.status != CHEM_ENUMERATED || first < 0) return;
    int64_t idx = first;
    for (int e = p.n_elems - 1; e >= 0; --e) {
        const int dgt = (int)(idx % p.radix[e]);
        idx /= p.radix[e];
        first_ox[e] = T.ox[p.elems[e] * CHEM_MAX_STATES + dgt];
    }
}

// The state of an atom of type z under first_ox (0 when its crystal has none; z is one of the plan's elements or the plan is not ENUMERATED).
CHEM_HD int chem_atom_state(const ChemPlan& p, const int* first_ox, int z) {
    int o = 0;
    const int E = p.n_elems < CHEM_MAX_ELEMS ? p.n_elems : CHEM_MAX_ELEMS;
    for (int e = 0; e < E; ++e)
        if (p.elems[e] == z) o = first_ox[e];
    return o;
}

}  // namespace mi
