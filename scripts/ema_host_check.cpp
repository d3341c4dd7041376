// The decay schedule of the weight average (matinvent_amd/csrc/ema_decay.h: what mi_adam_step_ema's host side and every wave of its
// guarded kernel run) compiled for the host and printed, so that a test can hold it to numpy and the host sanitizers see it run:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/ema_host_check.cpp -o ema_host_check
//   ./ema_host_check DECAY WARMUP S [S ...]
//
// One line per S: "S BITS VALUE" with BITS the float's 32 bits in hexadecimal and VALUE in %.9g.  DECAY is rounded to float as it is
// when it crosses the C boundary.  Exit status 2 for a malformed command line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../matinvent_amd/csrc/ema_decay.h"

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s DECAY WARMUP S [S ...]\n", argv[0]);
        return 2;
    }
    const float decay = (float)std::strtod(argv[1], nullptr);
    const int warmup = std::atoi(argv[2]);
    std::vector<unsigned> steps;   // (exactly argc - 3 values: the sanitizers see an index past the end)
    for (int k = 3; k < argc; ++k) steps.push_back((unsigned)std::strtoul(argv[k], nullptr, 10));
    for (size_t k = 0; k < steps.size(); ++k) {
        const float d = mi::ema_decay_at(decay, warmup, steps[k]);
        uint32_t bits;
        std::memcpy(&bits, &d, sizeof bits);
        std::printf("%u %08x %.9g\n", steps[k], (unsigned)bits, (double)d);
    }
    return 0;
}
