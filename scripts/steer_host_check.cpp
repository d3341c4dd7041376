// The resampling plan of a particle group (matinvent_amd/csrc/steer_plan.h: what lane 0 of steer_plan_kernel runs) compiled for the host
// and held to a plain restatement -- weights, sums and a search from the start for every offspring -- so that the host sanitizers see
// every index it forms:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/steer_host_check.cpp -o steer_host_check
//   ./steer_host_check [ROUNDS [SEED]]
//
// Every round draws a group: K in 1..256 (1, 2, 255 and 256 among them), scores with NaN / +-inf members, previous scores and log-weights
// with -inf members, all-NaN groups, bit-equal weights, lambda up to 1e4, ess_frac in {-1, 0.5, 2}.  The arrays are heap blocks of exactly
// K elements.  Compared bit for bit: ancestors, u_prev, logw, ESS and the flags.  Prints one summary line; exit status 1 on a mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../matinvent_amd/csrc/steer_plan.h"

static uint64_t rng_state;
static uint32_t rnd() {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 32);
}
static float unif() { return (float)(rnd() >> 8) * 5.9604644775390625e-8f; }

// the plain loop: same arithmetic and order of summation, a search from k = 0 for every offspring
static int plain(int K, const std::vector<float>& u, const std::vector<float>& lw, float ess_frac, float U, std::vector<int>& anc,
                 std::vector<float>& up, std::vector<float>& lo, float* ess) {
    for (int k = 0; k < K; ++k) anc[(size_t)k] = k;
    *ess = 0.f;
    float m = -INFINITY;
    for (int k = 0; k < K; ++k)
        if (lw[(size_t)k] > m) m = lw[(size_t)k];
    if (m == -INFINITY) return mi::STEER_NO_FINITE;
    std::vector<float> w((size_t)K), c((size_t)K);
    float S = 0.f, Q = 0.f;
    bool equal = true;
    int last = 0;
    for (int k = 0; k < K; ++k) {
        const float d = lw[(size_t)k] - m;
        w[(size_t)k] = lw[(size_t)k] == -INFINITY ? 0.f : expf(d);
        S = S + w[(size_t)k];
        c[(size_t)k] = S;
        const float v2 = w[(size_t)k] * w[(size_t)k];
        Q = Q + v2;
        if (w[(size_t)k] > 0.f) last = k;
        if (std::memcmp(&w[(size_t)k], &w[0], sizeof(float)) != 0) equal = false;
    }
    const float S2 = S * S;
    *ess = S2 / Q;
    const float limit = ess_frac * (float)K;
    if (!(ess_frac < 0.f || *ess < limit)) {
        for (int k = 0; k < K; ++k) {
            up[(size_t)k] = u[(size_t)k];
            lo[(size_t)k] = lw[(size_t)k];
        }
        return 0;
    }
    if (!equal)
        for (int j = 0; j < K; ++j) {
            const float a = U + (float)j;
            const float f = a / (float)K;
            const float t = f * S;
            int k = 0;
            while (k < last && !(c[(size_t)k] > t)) ++k;
            anc[(size_t)j] = k;
        }
    for (int k = 0; k < K; ++k) {
        lo[(size_t)k] = 0.f;
        up[(size_t)k] = u[(size_t)anc[(size_t)k]];
    }
    return mi::STEER_RESAMPLED;
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 2000;
    rng_state = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    if (rounds < 1) {
        std::fprintf(stderr, "usage: %s [ROUNDS [SEED]]\n", argv[0]);
        return 2;
    }
    const int fixedK[] = {1, 2, 255, 256, 64, 65};
    long resampled = 0, dead = 0, ident = 0;
    for (int r = 0; r < rounds; ++r) {
        const int K = r < 6 ? fixedK[r] : 1 + (int)(rnd() % 256);
        const int kind = (int)(rnd() % 8);   // 0: all NaN; 1: bit-equal; 2: lambda 1e4; else: mixed
        const int mode = (int)(rnd() % 3);
        const float lambda = kind == 2 ? 1e4f : 4.f * unif();
        const float fr[3] = {-1.f, 0.5f, 2.f};
        const float ess_frac = fr[rnd() % 3], target = unif() - 0.5f, U = unif();
        // heap blocks of exactly K elements: an index past the end is the sanitizer's to report
        std::vector<float> u((size_t)K), lw((size_t)K), w((size_t)K), up((size_t)K), lo((size_t)K), up2, lo2;
        std::vector<int> anc((size_t)K), anc2((size_t)K);
        for (int k = 0; k < K; ++k) {
            float o = 2.f * unif() - 1.f;
            const uint32_t q = rnd() % 16;
            if (kind == 0 || q == 0) o = NAN;
            else if (q == 1) o = INFINITY;
            else if (q == 2) o = -INFINITY;
            if (kind == 1) o = 0.25f;
            const float pv = kind == 1 ? 0.5f : (rnd() % 32 == 0 ? NAN : 2.f * unif() - 1.f);
            const float lg = kind == 1 ? 0.f : (rnd() % 32 == 0 ? -INFINITY : unif() - 0.5f);
            u[(size_t)k] = mi::steer_score(o, mode, target);
            up[(size_t)k] = pv;
            lo[(size_t)k] = lg;
            lw[(size_t)k] = mi::steer_logweight(lg, lambda, u[(size_t)k], pv);
        }
        up2 = up;
        lo2 = lo;
        float e1 = -1.f, e2 = -1.f;
        const int f1 = mi::steer_plan_group(K, u.data(), lw.data(), ess_frac, U, w.data(), anc.data(), up.data(), lo.data(), &e1);
        const int f2 = plain(K, u, lw, ess_frac, U, anc2, up2, lo2, &e2);
        bool ok = f1 == f2 && std::memcmp(&e1, &e2, sizeof e1) == 0 && anc == anc2 &&
                  std::memcmp(up.data(), up2.data(), (size_t)K * sizeof(float)) == 0 && std::memcmp(lo.data(), lo2.data(), (size_t)K * sizeof(float)) == 0;
        for (int k = 0; k < K && ok; ++k) ok = anc[(size_t)k] >= 0 && anc[(size_t)k] < K;
        if (kind == 1)
            for (int k = 0; k < K && ok; ++k) ok = anc[(size_t)k] == k;
        if (!ok) {
            std::printf("MISMATCH round %d K %d kind %d mode %d flags %d / %d ess %.9g / %.9g\n", r, K, kind, mode, f1, f2, (double)e1, (double)e2);
            return 1;
        }
        resampled += (f1 & mi::STEER_RESAMPLED) != 0;
        dead += (f1 & mi::STEER_NO_FINITE) != 0;
        bool id = true;
        for (int k = 0; k < K; ++k) id = id && anc[(size_t)k] == k;
        ident += id;
    }
    std::printf("steer_host_check: %d rounds, %ld resampled, %ld without a finite weight, %ld identities: OK\n", rounds, resampled, dead, ident);
    return 0;
}
