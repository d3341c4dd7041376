// The arithmetic of mi_relax_step (matinvent_amd/csrc/relax_fire.h: what relax_step_kernel calls) compiled for the host and held to a plain
// restatement -- one loop over the crystals with the formulas of include/matinvent_hip_relax.h written out -- so that the host sanitizers
// see every index it forms:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all scripts/relax_host_check.cpp -o relax_host_check
//   ./relax_host_check [ROUNDS [SEED]]
//
// Every round draws a ragged batch -- 1..6 crystals of 1..9 atoms, with and without relax_cell / per_atom / an explicit cell_factor, a
// near-singular lattice or a NaN / +-inf member of a gradient, the output or the lattice in some crystals, some crystals frozen beforehand
// -- and walks it through 12 consecutive steps on gradients that pull towards a drawn target, so that both signs of F.v, the growth of dt
// with its cap, the clamp and convergence all occur.  The arrays are heap blocks of exactly the batch's size.  Compared bit for bit after
// every step: coordinates, lattices, both velocity arrays and both state blocks.  Prints one summary line; exit status 1 on a mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../matinvent_amd/csrc/relax_fire.h"

static uint64_t rng_state;
static uint32_t rnd() {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 32);
}
static float unif() { return (float)(rnd() >> 8) * 5.9604644775390625e-8f; }
static float sym() { return 2.f * unif() - 1.f; }

typedef std::vector<float> vf;
typedef std::vector<int> vi;

static float plain_mod1(float x) {
    float r = fmodf(x, 1.0f);
    if (r < 0.f) r += 1.0f;
    return r;
}
// the tree of the header's comment: strides half(R), half(R) / 2, ..., 1
static float plain_tree(vf a) {
    const int R = (int)a.size();
    int p2 = 1;
    while (p2 < R) p2 *= 2;
    for (int s = p2 / 2; s >= 1; s /= 2)
        for (int i = 0; i < s && i + s < R; ++i) a[(size_t)i] = a[(size_t)i] + a[(size_t)(i + s)];
    return a[0];
}
static float d3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the plain loop: one crystal
static void plain_step(int n, const mi::RelaxParams& p, float* x, float* L, float* vx, float* vl, float* fs, int* is, const float* gx, const float* gl,
                       float out_p) {
    if (is[0] != 0) return;
    bool ok = std::isfinite(out_p);
    for (int q = 0; q < 9; ++q) ok = ok && std::isfinite(gl[q]) && std::isfinite(L[q]);
    for (int i = 0; i < 3 * n; ++i) ok = ok && std::isfinite(gx[i]);
    const float det = (L[0] * (L[4] * L[8] - L[5] * L[7]) + L[1] * (L[5] * L[6] - L[3] * L[8])) + L[2] * (L[3] * L[7] - L[4] * L[6]);
    if (!ok || !(std::fabs(det) >= p.det_min)) {
        is[0] = 2;
        return;
    }
    const float Li[9] = {(L[4] * L[8] - L[5] * L[7]) / det, (L[2] * L[7] - L[1] * L[8]) / det, (L[1] * L[5] - L[2] * L[4]) / det,
                         (L[5] * L[6] - L[3] * L[8]) / det, (L[0] * L[8] - L[2] * L[6]) / det, (L[2] * L[3] - L[0] * L[5]) / det,
                         (L[3] * L[7] - L[4] * L[6]) / det, (L[1] * L[6] - L[0] * L[7]) / det, (L[0] * L[4] - L[1] * L[3]) / det};
    const float s = p.per_atom ? p.scale * (float)n : p.scale, c = p.cell_factor > 0.f ? p.cell_factor : (float)n;
    const int R = p.relax_cell ? n + 3 : n;
    vf F((size_t)R * 3), V((size_t)R * 3);
    for (int r = 0; r < R; ++r)
        for (int k = 0; k < 3; ++k) {
            F[(size_t)(3 * r + k)] = r < n ? -(s * d3(gx + 3 * r, Li + 3 * k)) : -(s * gl[3 * (r - n) + k]) / c;
            V[(size_t)(3 * r + k)] = r < n ? vx[3 * r + k] : vl[3 * (r - n) + k];
        }
    vf pw((size_t)R), vv((size_t)R), ff((size_t)R);
    float fm2 = 0.f;
    for (int r = 0; r < R; ++r) {
        pw[(size_t)r] = d3(&F[(size_t)(3 * r)], &V[(size_t)(3 * r)]);
        vv[(size_t)r] = d3(&V[(size_t)(3 * r)], &V[(size_t)(3 * r)]);
        ff[(size_t)r] = d3(&F[(size_t)(3 * r)], &F[(size_t)(3 * r)]);
        fm2 = fmaxf(fm2, ff[(size_t)r]);
    }
    if (is[2] == 0) fs[2] = out_p;
    fs[3] = out_p;
    fs[4] = sqrtf(fm2);
    if (fs[4] < p.fmax) {
        is[0] = 1;
        return;
    }
    const float P = plain_tree(pw), nv = sqrtf(plain_tree(vv)), nf = sqrtf(plain_tree(ff));
    float dt = fs[0], al = fs[1];
    if (P > 0.f) {
        const float c1 = 1.0f - al, c2 = al * (nv / nf);
        for (size_t i = 0; i < V.size(); ++i) V[i] = c1 * V[i] + c2 * F[i];
        if (is[1] > p.n_min) {
            dt = fminf(dt * p.f_inc, p.dt_max);
            al = al * p.f_a;
        }
        is[1] += 1;
    } else {
        for (auto& v : V) v = 0.f;
        al = p.a_start;
        dt = dt * p.f_dec;
        is[1] = 0;
    }
    vf dr((size_t)R * 3), d2((size_t)R);
    for (size_t i = 0; i < V.size(); ++i) {
        V[i] = V[i] + dt * F[i];
        dr[i] = dt * V[i];
    }
    for (int r = 0; r < R; ++r) d2[(size_t)r] = d3(&dr[(size_t)(3 * r)], &dr[(size_t)(3 * r)]);
    const float nd = sqrtf(plain_tree(d2));
    const float k = nd > p.maxstep ? p.maxstep / nd : 1.0f;
    for (auto& v : dr) v = v * k;
    for (int r = 0; r < R; ++r)
        for (int q = 0; q < 3; ++q) {
            if (r < n) {
                vx[3 * r + q] = V[(size_t)(3 * r + q)];
                x[3 * r + q] = plain_mod1(x[3 * r + q] + ((dr[(size_t)(3 * r)] * Li[q] + dr[(size_t)(3 * r + 1)] * Li[3 + q]) + dr[(size_t)(3 * r + 2)] * Li[6 + q]));
            } else {
                vl[3 * (r - n) + q] = V[(size_t)(3 * r + q)];
                L[3 * (r - n) + q] = L[3 * (r - n) + q] + dr[(size_t)(3 * r + q)] / c;
            }
        }
    fs[0] = dt, fs[1] = al, fs[5] = nd;
    is[2] += 1;
}

template <typename T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T))); }

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 1000;
    rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    long bad = 0, count[4] = {0, 0, 0, 0}, neg = 0, grew = 0, capped = 0, clamped = 0;
    for (int r = 0; r < rounds; ++r) {
        const int B = 1 + (int)(rnd() % 6);
        vi off((size_t)B + 1, 0);
        for (int b = 0; b < B; ++b) off[(size_t)b + 1] = off[(size_t)b] + 1 + (int)(rnd() % 9);
        const int N = off[(size_t)B];
        mi::RelaxParams p;
        p.dt = 0.1f, p.dt_max = (rnd() & 1) ? 0.06f : 1.0f, p.maxstep = (rnd() & 1) ? 0.02f : 0.2f, p.f_inc = 1.1f, p.f_dec = 0.5f, p.a_start = 0.1f, p.f_a = 0.99f;
        p.fmax = (rnd() & 1) ? 0.5f : 0.02f, p.scale = 0.5f + unif(), p.cell_factor = (rnd() & 1) ? 0.f : 2.5f, p.det_min = 1e-3f;
        p.n_min = (int)(rnd() % 3), p.relax_cell = (int)(rnd() & 1), p.per_atom = (int)(rnd() & 1);
        vf x((size_t)N * 3), xt((size_t)N * 3), L((size_t)B * 9), Lt((size_t)B * 9), vx((size_t)N * 3, 0.f), vl((size_t)B * 9, 0.f), fs((size_t)B * mi::RELAX_NF, 0.f);
        vi is((size_t)B * mi::RELAX_NI, 0);
        for (auto& v : x) v = unif();
        for (size_t i = 0; i < x.size(); ++i) xt[i] = x[i] + 0.05f * sym();
        for (int b = 0; b < B; ++b) {
            for (int q = 0; q < 9; ++q) {
                Lt[(size_t)b * 9 + q] = (q % 4 == 0 ? 4.f + unif() : 0.3f * sym());
                L[(size_t)b * 9 + q] = Lt[(size_t)b * 9 + q] + 0.1f * sym();
            }
            fs[(size_t)b * mi::RELAX_NF] = p.dt, fs[(size_t)b * mi::RELAX_NF + 1] = p.a_start;
            const uint32_t k = rnd() % 12;
            if (k == 0) is[(size_t)b * mi::RELAX_NI] = 1 + (int)(rnd() % 3);   // frozen beforehand
            if (k == 1)
                for (int q = 0; q < 3; ++q) L[(size_t)b * 9 + 3 + q] = L[(size_t)b * 9 + q];   // two equal rows: det = 0
            if (k == 2) L[(size_t)b * 9 + rnd() % 9] = (rnd() & 1) ? NAN : INFINITY;
        }
        vf x2 = x, L2 = L, vx2 = vx, vl2 = vl, fs2 = fs;
        vi is2 = is;
        const float kx = 8.f + 8.f * unif(), kl = 1.f + unif();
        const int nan_step = (int)(rnd() % 24), nan_b = (int)(rnd() % (uint32_t)B), nan_what = (int)(rnd() % 3);
        for (int step = 0; step < 12; ++step) {
            // gradients of a quadratic about the targets, from the state of the header's run (both runs get the same arrays)
            vf gx((size_t)N * 3), gl((size_t)B * 9), out((size_t)B);
            for (size_t i = 0; i < gx.size(); ++i) gx[i] = kx * (x[i] - xt[i]);
            for (size_t i = 0; i < gl.size(); ++i) gl[i] = kl * (L[i] - Lt[i]);
            for (int b = 0; b < B; ++b) out[(size_t)b] = sym();
            if (step == nan_step) {
                const float nf = (rnd() & 1) ? NAN : -INFINITY;
                if (nan_what == 0) gx[(size_t)off[(size_t)nan_b] * 3 + rnd() % (uint32_t)((off[(size_t)nan_b + 1] - off[(size_t)nan_b]) * 3)] = nf;
                if (nan_what == 1) gl[(size_t)nan_b * 9 + rnd() % 9] = nf;
                if (nan_what == 2) out[(size_t)nan_b] = nf;
            }
            for (int b = 0; b < B; ++b) {
                const int o = off[(size_t)b], n = off[(size_t)b + 1] - o;
                vf work((size_t)(n + 3) * 4);
                const float dt0 = fs[(size_t)b * mi::RELAX_NF];
                const int st0 = is[(size_t)b * mi::RELAX_NI + 2], np0 = is[(size_t)b * mi::RELAX_NI + 1];
                mi::relax_step_crystal_host(n, p, x.data() + (size_t)o * 3, L.data() + (size_t)b * 9, vx.data() + (size_t)o * 3, vl.data() + (size_t)b * 9,
                                            fs.data() + (size_t)b * mi::RELAX_NF, is.data() + (size_t)b * mi::RELAX_NI, gx.data() + (size_t)o * 3,
                                            gl.data() + (size_t)b * 9, out[(size_t)b], work.data());
                plain_step(n, p, x2.data() + (size_t)o * 3, L2.data() + (size_t)b * 9, vx2.data() + (size_t)o * 3, vl2.data() + (size_t)b * 9,
                           fs2.data() + (size_t)b * mi::RELAX_NF, is2.data() + (size_t)b * mi::RELAX_NI, gx.data() + (size_t)o * 3, gl.data() + (size_t)b * 9,
                           out[(size_t)b]);
                if (is[(size_t)b * mi::RELAX_NI + 2] > st0) {   // a step was taken: which branches
                    const float dt1 = fs[(size_t)b * mi::RELAX_NF];
                    if (is[(size_t)b * mi::RELAX_NI + 1] == 0 && st0 > 0) ++neg;
                    if (dt1 > dt0) ++grew;
                    if (np0 > p.n_min && dt1 == p.dt_max) ++capped;
                    if (fs[(size_t)b * mi::RELAX_NF + 5] > p.maxstep) ++clamped;
                }
            }
            if (!same(x, x2) || !same(L, L2) || !same(vx, vx2) || !same(vl, vl2) || !same(fs, fs2) || !same(is, is2)) ++bad;
        }
        for (int b = 0; b < B; ++b) count[is[(size_t)b * mi::RELAX_NI] & 3]++;
        for (int b = 0; b < B; ++b)
            for (int i = off[(size_t)b] * 3; i < off[(size_t)b + 1] * 3; ++i)
                if (std::isfinite(x[(size_t)i]) && !(x[(size_t)i] >= 0.f && x[(size_t)i] <= 1.f)) ++bad;
    }
    printf("relax_host_check: %d rounds; crystals left active %ld, converged %ld, failed %ld, frozen as exhausted %ld; steps with F.v <= 0 %ld, dt grown %ld, "
           "dt at its cap %ld, clamped %ld; %ld mismatches\n", rounds, count[0], count[1], count[2], count[3], neg, grew, capped, clamped, bad);
    if (!(count[0] && count[1] && count[2] && neg && grew && capped && clamped)) {
        printf("relax_host_check: a branch was never taken\n");
        return 1;
    }
    return bad ? 1 : 0;
}
