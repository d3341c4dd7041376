// The latent columns of the crystal embedding (matinvent_amd/csrc/guidance_embed.h: what every thread of crystal_embedding_kernel runs for
// a property column) compiled for the host, held to a float64 formula over the whole input range, with the host sanitizers watching:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/guidance_host_check.cpp -o guidance_host_check
//   ./guidance_host_check [F [STEPS]]
//
// For every frequency w_k = (pi / 8) 2^k, k < F (default 12), and STEPS (default 20001) values of yhat spread over [-12, 12] -- the clamp
// range and beyond it on both sides -- plus the edge values 0, -0, +-8, +-nextafter(8), +-FLT_MAX, +-inf: the float32 column against
// sin / cos of (double)w_k * clamp(yhat) in float64.  The float32 product rounds the argument by at most half an ulp of 2048 pi (2.4e-4)
// before the sine sees it, so the bound is that half ulp plus the library's few ulp of the result; the column index map is checked
// against its inverse for every F.  Prints the largest deviation per frequency; exit status 1 on a miss, 2 for a bad command line.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../matinvent_amd/csrc/guidance_embed.h"

int main(int argc, char** argv) {
    const int F = argc > 1 ? std::atoi(argv[1]) : 12;
    const int steps = argc > 2 ? std::atoi(argv[2]) : 20001;
    if (F < 1 || F > 12 || steps < 2 || argc > 3) {
        std::fprintf(stderr, "usage: %s [F in 1..12 [STEPS >= 2]]\n", argv[0]);
        return 2;
    }
    std::vector<float> ys;   // (exactly the values pushed: the sanitizers see an index past the end)
    for (int i = 0; i < steps; ++i) ys.push_back((float)(-12.0 + 24.0 * (double)i / (double)(steps - 1)));
    const float edge[] = {0.0f, -0.0f, 8.0f, -8.0f, std::nextafterf(8.0f, 9.0f), std::nextafterf(8.0f, 0.0f), -std::nextafterf(8.0f, 9.0f),
                          FLT_MAX, -FLT_MAX, INFINITY, -INFINITY};
    for (float e : edge) ys.push_back(e);
    int bad = 0;
    for (int k = 0; k < F; ++k) {
        const float w = (float)(3.14159265358979323846 / 8.0 * (double)(1 << k));
        const double bound = 0.5 * (double)w * 8.0 * (double)FLT_EPSILON + 8.0 * (double)FLT_EPSILON;   // half an ulp of the argument, a few ulp of the result
        double worst = 0.0;
        for (size_t i = 0; i < ys.size(); ++i) {
            const float y = ys[i];
            const double yc = y < -8.0f ? -8.0 : (y > 8.0f ? 8.0 : (double)y);
            if ((double)mi::guidance_clamp(y) != yc) {
                std::printf("clamp(%.9g) = %.9g\n", (double)y, (double)mi::guidance_clamp(y));
                ++bad;
            }
            const double ds = std::fabs((double)mi::guidance_latent_column(y, w, false) - std::sin((double)w * yc));
            const double dc = std::fabs((double)mi::guidance_latent_column(y, w, true) - std::cos((double)w * yc));
            worst = std::fmax(worst, std::fmax(ds, dc));
        }
        std::printf("k = %2d  w = %.9g  max |float32 - float64| = %.3e  (bound %.3e)\n", k, (double)w, worst, bound);
        if (!(worst <= bound)) ++bad;
    }
    for (int f = 1; f <= 12; ++f)
        for (int P = 1; P <= 3; ++P)
            for (int j = 0; j < 2 * f * P; ++j) {
                int p, k;
                bool cosine;
                mi::guidance_column_index(j, f, &p, &k, &cosine);
                if (p < 0 || p >= P || k < 0 || k >= f || p * 2 * f + (cosine ? f : 0) + k != j) {
                    std::printf("column %d of F = %d: p = %d, k = %d, cosine = %d\n", j, f, p, k, (int)cosine);
                    ++bad;
                }
            }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
