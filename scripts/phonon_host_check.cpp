// The arithmetic of the phonon kernels on the host (matinvent_amd/csrc/phonon_fc.h with vib_dynmat.h and sym_jacobi.h): a
// stand-alone program that runs the headers in the kernels' order -- force constants, dynamical matrices, eigenvalues, thermodynamics --
// on the crystals of a case file and writes every intermediate, for tests/test_phonon_host.py to hold to the numpy restatement bit for
// bit.  Built on the CPU under the host sanitizers:
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all scripts/phonon_host_check.cpp -o phonon_host_check
//     phonon_host_check case.bin out.bin
// Case file: int32 B, K; double h, tie_tol, det_min, nu_cut, temps[8]; then per crystal: int32 Ns, reps[3], Q; float frac[Ns][3], lat[9];
// double mass[Ns], Gc[6 n][3 Ns] (n = Ns / N; nothing when reps does not divide Ns), table[Q][6 (a + b + c)]; int32 weight[Q].  Output per
// crystal (n = 0 when reps does not divide): int32 fc status; double asym, Phi[3 n][3 Ns]; int32 masks[n][Ns]; per q: double E[6 n][6 n],
// herm, evals[6 n]; int32 sweeps, eig status; then double lam[Q][3 n], freqs[Q][3 n], c_v[K], zpe, min_freq, herm, pair_gap; int32 n_imag,
// n_zero, min_q, sweeps_max, status.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../matinvent_amd/csrc/phonon_fc.h"

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
    double par[4], temps[VIB_MAX_TEMPS];
    rd(in, head, 2);
    rd(in, par, 4);
    rd(in, temps, (size_t)VIB_MAX_TEMPS);
    const int B = head[0], K = head[1];
    const double h = par[0], tie_tol = par[1], det_min = par[2], nu_cut = par[3];
    if (B < 0 || K < 1 || K > VIB_MAX_TEMPS) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    int total_sweeps = 0, bad = 0, items = 0;
    for (int b = 0; b < B; ++b) {
        int hd[5];
        rd(in, hd, 5);
        const int Ns = hd[0], reps[3] = {hd[1], hd[2], hd[3]}, Q = hd[4];
        if (Ns < 1 || Ns > VIB_MAX_ATOMS || reps[0] < 1 || reps[1] < 1 || reps[2] < 1 || Q < 1) {
            fprintf(stderr, "crystal %d: Ns = %d, reps = (%d, %d, %d), Q = %d\n", b, Ns, reps[0], reps[1], reps[2], Q);
            return 2;
        }
        const int N = ph_images(reps), n = (Ns % N == 0 && Ns / N <= PH_MAX_PRIM) ? Ns / N : 0, m = 3 * n, M = 6 * n;
        const size_t total = (size_t)9 * n * Ns, tl = (size_t)ph_table_len(reps);
        std::vector<float> frac((size_t)3 * Ns), lat(9);
        std::vector<double> mass((size_t)Ns), Gc(2 * total), Phi(total), table((size_t)Q * tl), E((size_t)M * M), Ew((size_t)M * M), evals((size_t)Q * M),
            lam((size_t)Q * m), nu((size_t)Q * m), cv((size_t)K), herm((size_t)Q);
        std::vector<int> masks((size_t)n * Ns), weight((size_t)Q), item_q((size_t)Q), sweeps((size_t)Q), est((size_t)Q);
        std::vector<int64_t> ev_off((size_t)Q);
        rd(in, frac.data(), frac.size());
        rd(in, lat.data(), lat.size());
        rd(in, mass.data(), mass.size());
        rd(in, Gc.data(), Gc.size());
        rd(in, table.data(), table.size());
        rd(in, weight.data(), weight.size());
        double asym;
        const int fst = ph_fc_crystal_host(Ns, reps, Gc.data(), mass.data(), frac.data(), lat.data(), h, tie_tol, det_min, Phi.data(), masks.data(), &asym);
        wr(out, &fst, 1);
        wr(out, &asym, 1);
        wr(out, Phi.data(), Phi.size());
        wr(out, masks.data(), masks.size());
        const int np = (jac_even(M) / 2) + 1;
        std::vector<double> rc((size_t)np), rs((size_t)np), rpp((size_t)np), rqq((size_t)np);
        std::vector<int> rrot((size_t)np);
        int st = fst;
        for (int q = 0; q < Q; ++q) {   // phonon_dynmat_kernel and sym_eig_kernel, item by item
            item_q[q] = q, ev_off[q] = (int64_t)q * M;
            if (fst == VIB_OK) {
                ph_dynmat_item_host(n, Ns, reps, Phi.data(), masks.data(), mass.data(), table.data() + (size_t)q * tl, E.data(), &herm[q]);
            } else {
                for (size_t i = 0; i < E.size(); ++i) E[i] = jac_nan();
                herm[q] = jac_nan();
            }
            Ew = E;
            est[q] = jac_eigvals_host(M, Ew.data(), evals.data() + (size_t)q * M, &sweeps[q], rc.data(), rs.data(), rpp.data(), rqq.data(), rrot.data());
            if (st == VIB_OK && est[q] > st) st = est[q];
            wr(out, E.data(), E.size());
            wr(out, &herm[q], 1);
            wr(out, evals.data() + (size_t)q * M, (size_t)M);
            wr(out, &sweeps[q], 1);
            wr(out, &est[q], 1);
            total_sweeps += sweeps[q];
        }
        const bool ok = st == VIB_OK;   // phonon_thermo_kernel
        for (int q = 0; q < Q; ++q)
            for (int k = 0; k < m; ++k) {
                const double l = ok ? ph_pair_mean(evals.data() + (size_t)q * M, k) : jac_nan();
                lam[(size_t)q * m + k] = l, nu[(size_t)q * m + k] = ok ? vib_frequency(l) : jac_nan();
            }
        for (int k = 0; k < K; ++k) cv[k] = ok ? ph_cv(lam.data(), ev_off.data(), item_q.data(), weight.data(), 0, Q, m, nu_cut, temps[k]) : jac_nan();
        int ni = -1, nz = -1, min_q = -1, sw = ok ? 0 : -1;
        const double zpe = ok ? ph_zpe(lam.data(), ev_off.data(), item_q.data(), weight.data(), 0, Q, m, nu_cut, &ni, &nz) : jac_nan();
        const double lo = ok ? ph_min_freq(lam.data(), ev_off.data(), item_q.data(), 0, Q, m, &min_q) : jac_nan();
        const double gap = ok ? ph_pair_gap(evals.data(), ev_off.data(), 0, Q, m) : jac_nan();
        double hm = ok ? 0.0 : jac_nan();
        for (int q = 0; ok && q < Q; ++q) hm = herm[q] > hm ? herm[q] : hm, sw = sweeps[q] > sw ? sweeps[q] : sw;
        const int status = ok ? VIB_OK : st;
        wr(out, lam.data(), lam.size());
        wr(out, nu.data(), nu.size());
        wr(out, cv.data(), cv.size());
        wr(out, &zpe, 1);
        wr(out, &lo, 1);
        wr(out, &hm, 1);
        wr(out, &gap, 1);
        wr(out, &ni, 1);
        wr(out, &nz, 1);
        wr(out, &min_q, 1);
        wr(out, &sw, 1);
        wr(out, &status, 1);
        items += Q;
        bad += status != VIB_OK;
    }
    fclose(in);
    fclose(out);
    printf("%d crystals, %d items, %d sweeps, %d not OK\n", B, items, total_sweeps, bad);
    return 0;
}
