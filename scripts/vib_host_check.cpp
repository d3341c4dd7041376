// The arithmetic of the vibration kernels on the host (matinvent_amd/csrc/vib_dynmat.h and sym_jacobi.h): a stand-alone program
// that runs both headers in the kernels' order -- displace, collect, dynmat, eigenvalues, thermodynamics -- on the crystals of a case file
// and writes every intermediate, for tests/test_vib_host.py to hold to the numpy restatement bit for bit.  Built on the CPU under the host
// sanitizers:
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all scripts/vib_host_check.cpp -o vib_host_check
//     vib_host_check case.bin out.bin
// Case file: int32 B, per_atom, K; double h, scale, det_min, nu_cut, temps[8]; then per crystal: int32 n; float frac[n][3], lat[9],
// g[6 n][n][3]; double mass[n].  Output per crystal: float displaced[6 n][n][3]; double Gc[6 n][3 n]; int32 dyn status; double asym, R[M][M],
// evals[M]; int32 sweeps, eig status; double freqs[M], c_v[K], zpe; int32 n_imag, n_zero, status.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../matinvent_amd/csrc/vib_dynmat.h"

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
    int head[3];
    double par[4], temps[VIB_MAX_TEMPS];
    rd(in, head, 3);
    rd(in, par, 4);
    rd(in, temps, (size_t)VIB_MAX_TEMPS);
    const int B = head[0], per_atom = head[1], K = head[2];
    const double h = par[0], scale = par[1], det_min = par[2], nu_cut = par[3];
    if (B < 0 || K < 1 || K > VIB_MAX_TEMPS) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    int total_sweeps = 0, bad = 0;
    for (int b = 0; b < B; ++b) {
        int n;
        rd(in, &n, 1);
        if (n < 1 || n > VIB_MAX_ATOMS) {
            fprintf(stderr, "crystal %d: n = %d\n", b, n);
            return 2;
        }
        const int N3 = 3 * n, M = vib_modes(n);
        std::vector<float> frac((size_t)N3), lat(9), g((size_t)6 * n * N3), disp((size_t)6 * n * N3);
        std::vector<double> mass((size_t)n), Gc((size_t)6 * n * N3), W((size_t)N3 * N3), R((size_t)M * M), Rw((size_t)M * M), v((size_t)3 * N3),
            U((size_t)3 * N3), w((size_t)N3), ev((size_t)M), nu((size_t)M), cv((size_t)K);
        rd(in, frac.data(), frac.size());
        rd(in, lat.data(), lat.size());
        rd(in, g.data(), g.size());
        rd(in, mass.data(), mass.size());
        double Li[9];
        const bool ok = vib_lattice(lat.data(), det_min, Li);
        const double s = vib_scale(scale, per_atom, n);
        for (int c = 0; c < 6 * n; ++c) {   // vib_displace_kernel and vib_collect_kernel, copy by copy
            const int atom = c / 6, d = (c % 6) / 2, sg = c & 1;
            for (int i = 0; i < N3; ++i) {
                disp[(size_t)c * N3 + i] = (ok && i / 3 == atom) ? vib_displaced(frac[i], h, d, sg, i % 3, Li) : frac[i];
                Gc[(size_t)c * N3 + i] = ok ? vib_cart_grad(g.data() + (size_t)c * N3 + 3 * (i / 3), Li, s, i % 3) : jac_nan();
            }
        }
        double asym;
        const int dst = vib_dynmat_crystal_host(n, Gc.data(), mass.data(), h, R.data(), &asym, W.data(), v.data(), U.data(), w.data());
        Rw = R;
        const int np = (jac_even(M) / 2) + 1;
        std::vector<double> rc((size_t)np), rs((size_t)np), rpp((size_t)np), rqq((size_t)np);
        std::vector<int> rrot((size_t)np);
        int sweeps = 0;
        const int est = jac_eigvals_host(M, Rw.data(), ev.data(), &sweeps, rc.data(), rs.data(), rpp.data(), rqq.data(), rrot.data());
        const int fst = dst != VIB_OK ? dst : est;   // (vib_thermo_kernel's: one atom has no matrix element to carry a bad input)
        const bool fine = fst == VIB_OK;
        for (int k = 0; k < M; ++k) nu[k] = fine ? vib_frequency(ev[k]) : jac_nan();
        for (int k = 0; k < K; ++k) cv[k] = fine ? vib_cv(ev.data(), M, nu_cut, temps[k]) : jac_nan();
        int ni = -1, nz = -1;
        const double zpe = fine ? vib_zpe(ev.data(), M, nu_cut, &ni, &nz) : jac_nan();
        wr(out, disp.data(), disp.size());
        wr(out, Gc.data(), Gc.size());
        wr(out, &dst, 1);
        wr(out, &asym, 1);
        wr(out, R.data(), R.size());
        wr(out, ev.data(), ev.size());
        wr(out, &sweeps, 1);
        wr(out, &est, 1);
        wr(out, nu.data(), nu.size());
        wr(out, cv.data(), cv.size());
        wr(out, &zpe, 1);
        wr(out, &ni, 1);
        wr(out, &nz, 1);
        wr(out, &fst, 1);
        total_sweeps += sweeps;
        bad += fst != VIB_OK;
    }
    fclose(in);
    fclose(out);
    printf("%d crystals, %d sweeps, %d not OK\n", B, total_sweeps, bad);
    return 0;
}
