// The structure-fingerprint kernel's own source (matinvent_amd/csrc/fingerprint_body.h) run on the host: blockIdx and threadIdx are loop
// variables, a barrier is the end of a phase's thread loop, the LDS additions are plain additions.  Every array is allocated at exactly
// its size, so that the host sanitizers see any index past an end:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/fingerprint_host_check.cpp -o fingerprint_host_check
//   ./fingerprint_host_check batch.txt rows.bin
//
// batch.txt: "B N nbins r_max sigma", then B + 1 offsets, N atom types, 3 N coordinates, 9 B lattice entries (nan / inf are read as such).
// rows.bin receives out_fp [B][36 nbins] and out_info [B][4] as raw fp32, for a comparison with tests/fp_ref64.py.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../matinvent_amd/csrc/fingerprint_body.h"

using namespace mi;

int main(int argc, char** argv) {
    if (argc < 3) return std::fprintf(stderr, "usage: %s batch.txt rows.bin\n", argv[0]), 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return std::perror(argv[1]), 2;
    int B, N, nbins;
    float r_max, sigma;
    if (std::fscanf(f, "%d %d %d %f %f", &B, &N, &nbins, &r_max, &sigma) != 5) return 2;
    if (B < 0 || N < 0 || nbins < 1 || nbins > MI_FP_MAX_BINS) return std::fprintf(stderr, "bad header\n"), 2;
    std::unique_ptr<int[]> off(new int[B + 1]), types(new int[N]);
    std::unique_ptr<float[]> frac(new float[(size_t)N * 3]), lat(new float[(size_t)B * 9]);
    std::unique_ptr<float[]> fp(new float[(size_t)B * MI_FP_MAX_BLOCKS * nbins]), info(new float[(size_t)B * 4]);
    for (int k = 0; k <= B; ++k)
        if (std::fscanf(f, "%d", &off[k]) != 1) return 2;
    for (int k = 0; k < N; ++k)
        if (std::fscanf(f, "%d", &types[k]) != 1) return 2;
    for (int k = 0; k < 3 * N; ++k)
        if (std::fscanf(f, "%f", &frac[k]) != 1) return 2;
    for (int k = 0; k < 9 * B; ++k)
        if (std::fscanf(f, "%f", &lat[k]) != 1) return 2;
    std::fclose(f);
    if (off[0] != 0 || off[B] != N) return std::fprintf(stderr, "offsets do not cover the atoms\n"), 2;

    FpArgs a{off.get(), types.get(), frac.get(), lat.get(), fp.get(), info.get(), r_max, sigma, nbins};
    std::unique_ptr<FpShared> s(new FpShared);
    using Phase = void (*)(FpShared&, const FpArgs&, int, int);
    const Phase phases[] = {fp_phase_init, fp_phase_scan, fp_phase_verdict, fp_phase_accumulate, fp_phase_weigh, fp_phase_norm, fp_phase_store};
    for (int b = 0; b < B; ++b)
        for (Phase p : phases)
            for (int tid = 0; tid < FP_THREADS; ++tid) p(*s, a, b, tid);

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return std::perror(argv[2]), 2;
    std::fwrite(fp.get(), sizeof(float), (size_t)B * MI_FP_MAX_BLOCKS * nbins, o);
    std::fwrite(info.get(), sizeof(float), (size_t)B * 4, o);
    std::fclose(o);
    for (int b = 0; b < B; ++b) std::printf("crystal %d: species %g status %g norm %g images %g\n", b, info[b * 4], info[b * 4 + 1], info[b * 4 + 2], info[b * 4 + 3]);
    return 0;
}
