// The arithmetic of the elasticity kernels on the host (matinvent_amd/csrc/elastic_fit.h): a stand-alone program that runs the
// header in the kernels' order -- strain, collect, fit -- on the crystals of a case file and writes every output, for
// tests/test_elastic_host.py to hold to the numpy restatement bit for bit.  Built on the CPU under the host sanitizers:
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all scripts/elastic_host_check.cpp -o elastic_host_check
//     elastic_host_check case.bin out.bin
// Case file: int32 B, per_atom; double h, scale, det_min; then per crystal: int32 n; float lat[9], g_lat[13][9] (the gradient at each
// copy's strained lattice); int32 ist[13] (each copy's relaxation status, MI_RELAX_CONVERGED when the ions are clamped).
// Output per crystal: float lat'[13][9]; double rows[13][8], C[36], S[36], stress0[6], pressure, asym, asym_C, moduli[15], evals[6], cond;
// int32 n_negative, n_unrelaxed, status.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../matinvent_amd/csrc/elastic_fit.h"

using namespace mi;

template <class T>
static void rd(FILE* f, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
}
template <class T>
static void wr(FILE* f, const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "short write\n");
        exit(2);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s case.bin out.bin\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "cannot open the files\n");
        return 2;
    }
    int head[2];
    double par[3];
    rd(in, head, 2);
    rd(in, par, 3);
    const int B = head[0], per_atom = head[1];
    const double h = par[0], scale = par[1], det_min = par[2];
    if (B < 0) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    int counts[3] = {0, 0, 0};
    for (int b = 0; b < B; ++b) {
        int n;
        rd(in, &n, 1);
        if (n < 1) {
            fprintf(stderr, "crystal %d: n = %d\n", b, n);
            return 2;
        }
        std::vector<float> lat(9), g((size_t)ELASTIC_COPIES * 9), strained((size_t)ELASTIC_COPIES * 9);
        std::vector<int> ist((size_t)ELASTIC_COPIES);
        std::vector<double> rows((size_t)ELASTIC_COPIES * ELASTIC_ROW), C(36), S(36), stress0(6), moduli(15), evals(6), work((size_t)ELASTIC_WORK);
        rd(in, lat.data(), lat.size());
        rd(in, g.data(), g.size());
        rd(in, ist.data(), ist.size());
        double Li[9], asym = 0.0;
        const bool ok = vib_lattice(lat.data(), det_min, Li);
        const double s = vib_scale(scale, per_atom, n);
        for (int c = 0; c < ELASTIC_COPIES; ++c) {   // elastic_strain_kernel and elastic_collect_kernel, copy by copy
            for (int q = 0; q < 9; ++q) strained[(size_t)c * 9 + q] = ok ? ela_strained(lat.data(), h, c, q / 3, q % 3) : lat[q];
            double a;
            ela_collect_row(strained.data() + (size_t)c * 9, g.data() + (size_t)c * 9, s, det_min, ist[c], rows.data() + (size_t)c * ELASTIC_ROW, &a);
            if (c == ELASTIC_COPIES - 1) asym = a;
        }
        ElasticFit o;
        o.C = C.data(), o.S = S.data(), o.stress0 = stress0.data(), o.moduli = moduli.data(), o.evals = evals.data();
        ela_fit_crystal(rows.data(), h, work.data(), &o);
        if (o.status == ELASTIC_BAD_INPUT) asym = jac_nan();   // (elastic_fit_kernel's)
        wr(out, strained.data(), strained.size());
        wr(out, rows.data(), rows.size());
        wr(out, C.data(), C.size());
        wr(out, S.data(), S.size());
        wr(out, stress0.data(), stress0.size());
        wr(out, &o.pressure, 1);
        wr(out, &asym, 1);
        wr(out, &o.asym_C, 1);
        wr(out, moduli.data(), moduli.size());
        wr(out, evals.data(), evals.size());
        wr(out, &o.cond, 1);
        wr(out, &o.n_negative, 1);
        wr(out, &o.n_unrelaxed, 1);
        wr(out, &o.status, 1);
        counts[o.status] += 1;
    }
    fclose(in);
    fclose(out);
    printf("%d crystals: %d ok, %d bad input, %d singular\n", B, counts[0], counts[1], counts[2]);
    return 0;
}
