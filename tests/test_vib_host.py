"""CPU checks of the Gamma-point vibrations that need no GPU (matinvent_amd.vibrations, include/matinvent_hip_vib.h,
matinvent_amd/csrc/vib_dynmat.h and sym_jacobi.h): the header, its table and the build list; the numpy restatement
tests/vib_ref64.py against LAPACK, against mpmath at 50 digits and against closed forms; the kernels' text run on the host under the host
sanitizers and held to the restatement bit for bit; the case lists of tests/test_gpu_vib.py; the chunk plan, the supercell and the reward
calculator with the device call replaced."""
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest

from matinvent_amd import _lib
from tests import vib_ref64 as R
from tests.header_util import ROOT, declared_symbols

# the parameters of every synthetic case, here and in tests/test_gpu_vib.py
H, SCALE, PER_ATOM, TEMPS, NU_CUT = 0.01, 1.5, True, (300.0, 10.0, 1000.0), 0.05
ATOM_COUNTS = (1, 2, 3, 20, 43, 44)       # orders 0, 3, 6, 57, 126 (the largest in LDS), 129 (the smallest in global memory)
EIG_SIZES = (1, 2, 3, 57, 126, 129)

# |eigenvalue(Jacobi) - eigenvalue(reference)| in units of M 2^-53 |A|_2.  Measured on measure_set() -- the random matrices of
# eig_matrices, 200 more of orders 2 .. 12, and the vibrational matrices of every crystal of tests/test_gpu_vib.py: the restatement against
# mpmath.eigsy at 50 digits, orders <= 57: 1.20 at most (at orders 3 and 6, where the unit is below one ulp of the largest eigenvalue;
# 0.20 at orders 20 and 57; LAPACK's own deviation from mpmath on the same set: 2.6); against numpy.linalg.eigvalsh at orders 126 and
# 129: 0.31 at most.  The bound is 4 x the larger of the two.
EIGVALSH_BOUND = 4 * 1.20

# c_v / k_B = sum of (x / expm1(x)) (x / -expm1(-x)) over positive terms.  expm1 is the one operation whose last place differs between
# numpy, the host's C library and the device's: two expm1 values of at most 2 ulp each (the device library states 1 ulp, the C library
# less), two divisions and a product of half an ulp each on both sides, and a sum of positive terms, which keeps a relative error:
# 2 (2 + 2) + 3 = 11 half-ulps, taken as 8 x 2^-52.  Everything else -- sqrt and division included -- is held to equality.
CV_RTOL = 8 * 2.0 ** -52


def rand_sym(M, seed):
    a = np.random.default_rng(seed).standard_normal((M, M))
    return (a + a.T) * 0.5


@lru_cache(maxsize=None)
def eig_matrices():
    """EIG_SIZES random symmetric matrices, then: a diagonal one, kron(I_3, S), an empty one, one with an infinite element."""
    mats = [rand_sym(M, 500 + M) for M in EIG_SIZES]
    bad = rand_sym(4, 9)
    bad[1, 2] = bad[2, 1] = np.inf
    return mats + [np.diag(np.random.default_rng(5).standard_normal(7)), np.kron(np.eye(3), rand_sym(5, 6)), np.zeros((0, 0)), bad]


@lru_cache(maxsize=None)
def kernel_crystals():
    """One spring crystal per atom count, and one of isotropic springs (five atoms: four three-fold levels)."""
    return [R.make_springs(n, 100 + n) for n in ATOM_COUNTS] + [R.make_springs(5, 77, isotropic=True)]


@lru_cache(maxsize=None)
def grid_crystals():
    return [R.make_springs(1 + k % 3, 1000 + k) for k in range(300)]


@lru_cache(maxsize=None)
def measure_set():
    """The matrices EIGVALSH_BOUND was measured on."""
    vib = [R.analyze(sp, H, SCALE, PER_ATOM, TEMPS, NU_CUT)["R"] for sp in grid_crystals() + kernel_crystals() if sp["n"] > 1]
    return eig_matrices()[:len(EIG_SIZES)] + vib + [rand_sym(M, 7000 + 17 * M + k) for M in (2, 3, 4, 6, 12) for k in range(40)]


def unit(A):
    return A.shape[0] * 2.0 ** -53 * np.linalg.norm(A, 2)


def test_header_table_and_build_list():
    from matinvent_amd.build import SOURCES
    names = sorted(declared_symbols("matinvent_hip_vib.h"))
    assert names == ["mi_sym_eigvals", "mi_vib_collect", "mi_vib_displace", "mi_vib_dynmat", "mi_vib_run_chunk", "mi_vib_thermo", "mi_vib_workspace"]
    assert sorted(_lib.VIB_SIGNATURES) == names and any(t is _lib.VIB_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    assert "vib.hip" in SOURCES
    head = open(os.path.join(ROOT, "include", "matinvent_hip_vib.h")).read()
    dyn = open(os.path.join(ROOT, "matinvent_amd", "csrc", "vib_dynmat.h")).read()
    jac = open(os.path.join(ROOT, "matinvent_amd", "csrc", "sym_jacobi.h")).read()
    assert '#include "matinvent_hip_relax.h"' in head and "fp contract(off)" in dyn and "fp contract(off)" in jac
    for k, name in enumerate(("OK", "NO_CONVERGENCE", "BAD_INPUT")):
        assert f"#define MI_VIB_{name} {k}" in head and f"VIB_{name} = {k}" in dyn and f"EIG_{name} = {k}" in jac
    assert (_lib.VIB_OK, _lib.VIB_NO_CONVERGENCE, _lib.VIB_BAD_INPUT) == (R.OK, R.NO_CONVERGENCE, R.BAD_INPUT) == (0, 1, 2)
    for name, val in (("MI_VIB_MAX_ATOMS", 256), ("MI_VIB_MAX_TEMPS", 8), ("MI_EIG_MAX_SWEEPS", 30), ("MI_EIG_LDS_MAX_M", 128), ("MI_EIG_MAX_M", 768)):
        assert f"#define {name} {val}" in head
    assert (_lib.VIB_MAX_ATOMS, _lib.VIB_MAX_TEMPS, _lib.EIG_MAX_SWEEPS, _lib.EIG_LDS_MAX_M, _lib.EIG_MAX_M) == (R.MAX_ATOMS, R.MAX_TEMPS, R.MAX_SWEEPS, R.LDS_MAX_M, R.MAX_M) == (256, 8, 30, 128, 768)
    assert 8 * R.LDS_MAX_M ** 2 == 128 * 1024 and 3 * 43 - 3 <= R.LDS_MAX_M < 3 * 44 - 3
    assert "VIB_THZ = 15.633304" in dyn and R.THZ == 15.633304
    # CODATA 2018: e, u, h, k_B
    e, u, h, kB = 1.602176634e-19, 1.66053906660e-27, 6.62607015e-34, 1.380649e-23
    assert abs(np.sqrt(e / (u * 1e-20)) / (2 * np.pi) / 1e12 - R.THZ) < 5e-7
    assert abs(h / e * 1e12 / R.H_EV_THZ - 1) < 1e-15 and abs(h * 1e12 / kB / R.H_KB_THZ - 1) < 1e-15 and abs(kB * 6.02214076e23 / R.KB_J_MOL - 1) < 1e-15
    for f in ("vib_host_check.cpp",):
        assert os.path.exists(os.path.join(ROOT, "scripts", f))
    # the argument blocks are the header's structs, field for field
    for cls, struct in ((_lib.VibChunkArgs, "mi_vib_chunk_args"), (_lib.VibDynmatArgs, "mi_vib_dynmat_args"), (_lib.SymEigArgs, "mi_sym_eig_args"),
                        (_lib.VibThermoArgs, "mi_vib_thermo_args")):
        body = head[head.index(f"typedef struct {struct}"):head.index(f"}} {struct};")]
        at = -1
        for k, _ in cls._fields_:
            hits = [i for i in (body.find(f" {k};", at + 1), body.find(f"*{k};", at + 1), body.find(f" {k},", at + 1), body.find(f" {k}[", at + 1)) if i >= 0]
            assert hits and min(hits) > at, (struct, k)
            at = min(hits)
    # the entries bind, and their host-only refusals answer without a GPU
    lib = _lib.load()
    from matinvent_amd.vibrations import _ws_layout
    nbytes, off = _ws_layout([1, 2, 20])
    assert off.tolist() == [0, 27, 27 + 108 + 18, 27 + 126 + 27 * 400 + 2 * 57 * 57] and nbytes == 8 * off[-1]
    import ctypes as C
    assert lib.mi_vib_workspace((C.c_int * 1)(257), 1, None) == _lib.MI_EINVAL and b"257 atoms" in lib.mi_last_error()
    for fn in (lib.mi_vib_dynmat, lib.mi_sym_eigvals, lib.mi_vib_thermo):
        assert fn(None, None) == _lib.MI_EINVAL and b"null argument block" in lib.mi_last_error()
    assert lib.mi_vib_displace(None, None, None) == _lib.MI_EINVAL and b"null handle" in lib.mi_last_error()


def test_round_robin_visits_every_pair_once():
    for M in (1, 2, 3, 4, 7, 8, 57, 129):
        Me = M + (M & 1)
        seen = set()
        for r in range(Me - 1):
            p, q = R.pairs(Me, r)
            assert (p < q).all() and len(set(p.tolist()) | set(q.tolist())) == Me   # disjoint
            seen |= {(int(a), int(b)) for a, b in zip(p, q)}
        assert seen == {(a, b) for a in range(Me) for b in range(a + 1, Me)}


def test_restated_eigenvalues_against_lapack_and_mpmath():
    import mpmath
    worst_mp = worst_lap = 0.0
    for A in measure_set():
        M = A.shape[0]
        ev, sweeps, status = R.jacobi(A)
        assert status == R.OK and sweeps <= 14 and (np.diff(ev) >= 0).all()
        if M <= 57:
            mpmath.mp.dps = 50
            ref = np.array(sorted(float(x) for x in mpmath.eigsy(mpmath.matrix(A.tolist()), eigvals_only=True)))
            worst_mp = max(worst_mp, np.abs(ev - ref).max() / unit(A))
        else:
            worst_lap = max(worst_lap, np.abs(ev - np.linalg.eigvalsh(A)).max() / unit(A))
        assert np.abs(ev - np.linalg.eigvalsh(A)).max() <= EIGVALSH_BOUND * unit(A), M
    if os.environ.get("MI_TOL_REPORT"):
        print(f"TOL vib jacobi: restatement vs mpmath (M <= 57) {worst_mp:.3f}, vs eigvalsh (M > 57) {worst_lap:.3f} units of M 2^-53 |A|_2; bound {EIGVALSH_BOUND:g}")
    assert max(worst_mp, worst_lap) <= EIGVALSH_BOUND / 4 * 1.01   # the measurement the bound was taken from
    # the special ones: diagonal (no sweep), three-fold, empty, not finite
    diag, kron, empty, bad = eig_matrices()[len(EIG_SIZES):]
    ev, sweeps, status = R.jacobi(diag)
    assert sweeps == 0 and status == R.OK and np.array_equal(ev, np.sort(np.diag(diag)))
    ev, sweeps, status = R.jacobi(kron)
    assert status == R.OK and np.abs(ev.reshape(-1, 3) - np.linalg.eigvalsh(kron[:5, :5])[:, None]).max() <= EIGVALSH_BOUND * unit(kron)
    assert R.jacobi(empty) == (pytest.approx(np.zeros(0)), 0, R.OK)
    # a diagonal whose product overflows: the rotation test takes two roots, so the pair still rotates
    big = np.array([[1e200, 1e190], [1e190, -1e200]])
    ev, sweeps, status = R.jacobi(big)
    assert status == R.OK and sweeps >= 1 and np.abs(ev - np.linalg.eigvalsh(big)).max() <= EIGVALSH_BOUND * unit(big)
    ev, sweeps, status = R.jacobi(bad)
    assert status == R.BAD_INPUT and np.isnan(ev).all()


def _analytic(sp):
    """(D, its eigenvalues) of a spring crystal's analytic Hessian under SCALE and PER_ATOM."""
    Hs = R.spring_hessian(sp) * (SCALE * sp["n"] if PER_ATOM else SCALE)
    m = np.repeat(sp["mass"], 3)
    D = Hs / np.sqrt(m[:, None] * m[None, :])
    return D, np.linalg.eigvalsh(D)


def test_the_reduction_removes_three_exact_translations():
    """Fed the analytic Hessian (Gc rows +-h H: the central difference gives it back to rounding), the reflected matrix has three rows at
    rounding level and the reduced block has the non-zero spectrum of D.  Both bounds are the issue's prototype figures x 4: 1e-16 of max|D|
    for the rows, 1e-14 of |D|_2 for the spectrum (at 57 atoms; here 44 at most)."""
    for sp in kernel_crystals()[1:]:
        n = sp["n"]
        Hs = R.spring_hessian(sp)
        Gc = np.empty((6 * n, 3 * n))
        Gc[0::2], Gc[1::2] = H * Hs, -H * Hs
        st = {}
        status, Rm, asym = R.dynmat(Gc, sp["mass"], H, st)
        assert status == R.OK and asym < 1e-12
        D = st["D"]
        assert np.abs(st["QDQ"][:3]).max() <= 4e-16 * np.abs(D).max() * 3 * n and np.array_equal(Rm, Rm.T)
        ev = np.linalg.eigvalsh(D)
        assert np.abs(ev[:3]).max() <= 4e-14 * np.linalg.norm(D, 2)   # the acoustic sum rule holds: three zero modes
        assert np.abs(np.linalg.eigvalsh(Rm) - ev[3:]).max() <= 4e-14 * np.linalg.norm(D, 2), n
        assert ev[3] > 1e-3 * ev[-1]   # (and no fourth one: the springs hold every atom)


def test_the_whole_restatement_finds_the_analytic_spectrum():
    """From float32 gradients of displaced copies: the spectrum of the analytic D to the gradients' own rounding, 2^-24 |g| / (2 h) per
    Hessian element, i.e. 2^-24 max|g| / (2 h) x 3 n of |H|_2 at most (a norm bound), x 4."""
    for sp in kernel_crystals()[1:4] + kernel_crystals()[-1:]:
        n = sp["n"]
        g = R.spring_copies(sp, H)
        res = R.analyze(sp, H, SCALE, PER_ATOM, TEMPS, NU_CUT, g_copies=g)
        D, ev = _analytic(sp)
        s = SCALE * n if PER_ATOM else SCALE
        tol = 4 * 3 * n * 2.0 ** -24 * np.abs(g).max() * s / (2 * H) / sp["mass"].min() * 6.5   # (|g_cart| <= |g_frac| |L^-1|; cells of 5 .. 7.5 A: L^-1 below 1/4.8, and g_frac carries L: the factor 6.5 covers |L| |L^-1|)
        assert res["status"] == R.OK and np.abs(res["evals"] - ev[3:]).max() <= tol, (n, np.abs(res["evals"] - ev[3:]).max(), tol)
        assert res["n_imag"] == 0 and res["n_zero"] == 0 and res["asym"] < 1e-3


def test_heat_capacity_limits():
    lam = np.array([0.5, 1.0, 2.5, 2.5, 9.0])   # eV / (amu A^2): 11 .. 47 THz
    hot = R.thermo(lam, R.OK, (1e9,), NU_CUT)
    assert abs(hot["c_v"][0] - 5.0) < 1e-9 and hot["n_zero"] == 0
    cold = R.thermo(lam, R.OK, (1e-3, 1.0), NU_CUT)
    assert cold["c_v"][0] == 0.0 and 0.0 <= cold["c_v"][1] < 1e-200
    # a zero and an imaginary mode count and contribute nothing: c_v -> (M - n_zero - n_imag) k_B
    mixed = R.thermo(np.array([-4.0, 1e-9, 0.5, 1.0]), R.OK, (1e9,), NU_CUT)
    assert mixed["n_imag"] == 1 and mixed["n_zero"] == 1 and abs(mixed["c_v"][0] - 2.0) < 1e-9
    assert mixed["freqs"][0] == -2.0 * R.THZ and abs(mixed["zpe"] - 0.5 * R.H_EV_THZ * R.THZ * (np.sqrt(0.5) + 1.0)) < 1e-15
    # Einstein's function at x = 1
    x1 = R.thermo(np.array([(300.0 / R.H_KB_THZ / R.THZ) ** 2]), R.OK, (300.0,), NU_CUT)
    assert abs(x1["c_v"][0] - np.e / (np.e - 1) ** 2) < 1e-12
    failed = R.thermo(lam, R.NO_CONVERGENCE, (300.0,), NU_CUT)
    assert np.isnan(failed["c_v"]).all() and np.isnan(failed["zpe"]) and failed["n_imag"] == failed["n_zero"] == -1
    assert R.thermo(np.zeros(0), R.OK, (300.0,), NU_CUT)["c_v"][0] == 0.0   # one atom: every sum is exactly 0
    c_mol, c_g = R.molar(np.array([3.0]), 100.0)
    assert abs(c_mol[0] - 3 * 8.31446261815324) < 1e-12 and abs(c_g[0] - c_mol[0] / 100.0) < 1e-15


def test_two_atoms_and_one_spring():
    """lambda = k (1 / m1 + 1 / m2) on the bond axis, 0 across it."""
    k, m1, m2 = 3.0, 15.999, 55.845
    sp = dict(n=2, tau=np.array([[0.1, 0.2, 0.3], [0.3, 0.2, 0.3]]), frac=np.array([[0.1, 0.2, 0.3], [0.31, 0.2, 0.3]], np.float32),
              lat=(np.eye(3) * 5.0).astype(np.float32), K=np.zeros((2, 2, 3, 3)), mass=np.array([m1, m2]))
    sp["K"][0, 1] = sp["K"][1, 0] = np.diag([k, 0.0, 0.0])
    res = R.analyze(sp, H, 1.0, False, (300.0,), NU_CUT)
    want = k * (1 / m1 + 1 / m2)
    assert res["status"] == R.OK and res["n_zero"] == 2 and res["n_imag"] == 0
    assert abs(res["evals"][2] - want) <= 4 * 2.0 ** -24 * (k * 0.05 * 5.0) / (2 * H) / m1 * 3 and np.abs(res["evals"][:2]).max() < 1e-9


def test_a_supercell_has_the_cells_spectrum_inside():
    """structure.make_supercell, and the Gamma spectrum of a doubled cell: a chain of two masses along x with springs to both neighbours
    (the cell's own spring and the one through the boundary) has optical lambda = 2 k (1 / m1 + 1 / m2) at Gamma; the doubled cell's
    Gamma holds it and the zone-boundary pair 2 k / m1, 2 k / m2."""
    from matinvent_amd.data import SimpleStructure
    from matinvent_amd.structure import make_supercell
    s = SimpleStructure([4.0, 5.0, 6.0], [90.0, 90.0, 90.0], [8, 26], np.array([[0.0, 0.5, 0.5], [0.5, 0.5, 0.5]]))
    big = make_supercell(s, (2, 1, 1))
    assert big.lengths == [8.0, 5.0, 6.0] and big.species == [8, 26, 8, 26] and big.angles == [90.0, 90.0, 90.0]
    assert np.allclose(big.frac_coords, [[0.0, 0.5, 0.5], [0.25, 0.5, 0.5], [0.5, 0.5, 0.5], [0.75, 0.5, 0.5]])
    with pytest.raises(ValueError):
        make_supercell(s, (0, 1, 1))
    k, m = 2.0, np.array([15.999, 55.845])

    def chain(cells):
        n = 2 * cells
        Hx = np.zeros((n, n))
        for i in range(n):   # nearest neighbours along x, periodic
            for j in ((i + 1) % n, (i - 1) % n):
                Hx[i, j] -= k
                Hx[i, i] += k
        Hs = np.zeros((3 * n, 3 * n))
        Hs[0::3, 0::3] = Hx
        Gc = np.empty((6 * n, 3 * n))
        Gc[0::2], Gc[1::2] = H * Hs, -H * Hs
        status, Rm, _ = R.dynmat(Gc, np.tile(m, cells), H)
        ev, _, est = R.jacobi(Rm)
        assert status == est == R.OK
        return ev

    one, two = chain(1), chain(2)
    opt = 2 * k * (1 / m[0] + 1 / m[1])
    assert abs(one[-1] - opt) < 1e-12 and np.abs(one[:-1]).max() < 1e-12
    for lam in (opt, 2 * k / m[0], 2 * k / m[1]):
        assert np.abs(two - lam).min() < 1e-12, lam


def test_chunk_plan():
    from matinvent_amd.vibrations import chunk_plan
    for na, bs in (([1, 2, 3], 7), ([2, 3], 1), ([20] * 4, 256), ([], 5), ([3], 1000)):
        got = chunk_plan(na, bs)
        want = R.chunk_plan(na, bs)
        assert len(got) == len(want) == -(-6 * sum(na) // bs)
        for (s, c), w in zip(got, want):
            assert s.dtype == c.dtype == np.int32 and list(zip(s.tolist(), c.tolist())) == w and 1 <= len(w) <= bs
    # equal atom-count lists in consecutive chunks (one handle) whenever the chunk holds whole crystals of one size
    lists = [[20] * len(s) for s, _ in chunk_plan([20] * 4, 120)]
    assert lists == [[20] * 120] * 4


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("vib") / "vib_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "vib_host_check.cpp"), "-o", exe], check=True)
    return exe


def test_host_check_under_the_host_sanitizers(host_check, tmp_path):
    """scripts/vib_host_check.cpp: both headers in the kernels' order, built with AddressSanitizer and UndefinedBehaviorSanitizer as a
    stand-alone program -- equal to the restatement in every output, bit for bit, on the crystals of tests/test_gpu_vib.py, on a slice of
    the grid, with a NaN gradient element and with a singular lattice, each also in a crystal of one atom."""
    crystals = kernel_crystals() + grid_crystals()[:30]
    flat = dict(kernel_crystals()[2], lat=np.zeros((3, 3), np.float32))
    one_flat = dict(kernel_crystals()[0], lat=np.zeros((3, 3), np.float32))   # ONE atom: no matrix element carries the bad input to the solver
    crystals = crystals + [flat, one_flat, grid_crystals()[0]]
    assert crystals[-1]["n"] == crystals[-2]["n"] == 1
    g = [R.spring_copies(sp, H) for sp in crystals]
    g[3] = g[3].copy()
    g[3][5, 7, 1] = np.nan
    g[-1] = g[-1].copy()
    g[-1][2, 0, 1] = np.nan
    cf, of = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    R.write_case(cf, crystals, g, H, SCALE, PER_ATOM, 1e-3, NU_CUT, TEMPS)
    r = subprocess.run([host_check, cf, of], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = R.read_out(of, [sp["n"] for sp in crystals], len(TEMPS))
    same = lambda a, b: np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    for b, (sp, gg, o) in enumerate(zip(crystals, g, got)):
        ref = R.analyze(sp, H, SCALE, PER_ATOM, TEMPS, NU_CUT, g_copies=gg)
        disp = np.stack([R.displace(sp["frac"], sp["lat"], c, H) for c in range(6 * sp["n"])])
        assert same(disp, o["displaced"]), b
        for k in ("Gc", "R", "asym", "evals", "freqs", "zpe"):
            assert same(ref[k], o[k]), (b, sp["n"], k)
        assert same(np.isnan(ref["c_v"]), np.isnan(o["c_v"])) and not (np.abs(ref["c_v"] - o["c_v"]) > CV_RTOL * ref["c_v"]).any(), (b, ref["c_v"], o["c_v"])   # (expm1)
        assert (ref["sweeps"], ref["status"], ref["n_imag"], ref["n_zero"]) == (o["sweeps"], o["status"], o["n_imag"], o["n_zero"]), b
    assert got[3]["status"] == R.BAD_INPUT and got[-3]["status"] == R.BAD_INPUT and np.isnan(got[-3]["Gc"]).all()
    for o in got[-2:]:   # the one-atom crystals: nothing but the dynmat status says so
        assert o["status"] == o["dyn_status"] == R.BAD_INPUT and o["eig_status"] == R.OK and np.isnan(o["c_v"]).all() and np.isnan(o["zpe"]) and o["n_imag"] == o["n_zero"] == -1
    assert sum(o["status"] != R.OK for o in got) == 4 and f"{len(crystals)} crystals" in r.stdout and "4 not OK" in r.stdout


def test_the_reward_calculators_nan_rules(monkeypatch, tmp_path):
    from types import SimpleNamespace
    from matinvent_amd import rewards, vibrations
    pred = SimpleNamespace(names=["energy", "gap"], hparams={}, normalizer=SimpleNamespace(std=[1.0, 1.0]), P=2, device="cpu")
    calls = []

    def fake(v, records):
        calls.append((v, list(records)))
        n = len(records)
        return dict(status=np.array([0, 1, 2, -1, 0][:n]), n_imag=np.array([0, 0, 0, -1, 2][:n]), c_v_gram=np.arange(1.0, n + 1)[:, None] * np.ones((1, 1)))

    monkeypatch.setattr(vibrations, "analyze_records", fake)
    hc = rewards.HeatCapacity(predictor=pred, task="energy", temperature=250.0, supercell=(2, 1, 1), delta=0.02)
    out = hc.calc((list("abcde"), None))
    assert np.array_equal(out, [1.0, np.nan, np.nan, np.nan, 5.0], equal_nan=True)
    v = calls[0][0]
    assert v.temperatures == (250.0,) and v.supercell == (2, 1, 1) and v.delta == 0.02 and v.per_atom and v.p == 0
    strict = rewards.HeatCapacity(predictor=pred, task="energy", require_stable=True, relaxer=lambda s, p: (s[::-1], np.zeros(len(s))))
    out = strict.calc(list("abcde"))
    assert np.array_equal(out, [1.0, np.nan, np.nan, np.nan, np.nan], equal_nan=True) and calls[-1][1] == list("edcba")
    assert hc.calc([]).size == 0
    for bad in (dict(task=None), dict(task="energy", temperature=0.0), dict(task="energy", model_path="x")):
        with pytest.raises(ValueError):
            rewards.HeatCapacity(predictor=pred, **bad)
    with pytest.raises(ValueError):
        rewards.HeatCapacity(predictor=pred, task="volume")
    # through Reward: a failed structure gets reward 0
    rw = rewards.Reward(str(tmp_path / "rewards"), [dict(name="heat_capacity", calculator=hc, target="ascending", minv=0.0, maxv=10.0)], 0.8)
    r, props, failed = rw.scoring(list("abcde"))
    assert r.tolist() == [0.1, 0.0, 0.0, 0.0, 0.5] and failed.tolist() == [False, True, True, True, False]
    assert "out of scope" in rewards.__doc__ and "HeatCapacity" in rewards.__doc__ and "are out of scope (SURVEY" not in rewards.__doc__


def test_vibrations_refuses_bad_arguments():
    from types import SimpleNamespace
    from matinvent_amd.vibrations import Vibrations
    pred = SimpleNamespace(names=["energy"], hparams={}, normalizer=SimpleNamespace(std=[2.0]), P=1, device="cpu")
    v = Vibrations(pred, "energy")
    assert (v.delta, v.per_atom, v.temperatures, v.nu_cut, v.batch_size, v.supercell) == (0.01, True, (300.0,), 0.05, 256, (1, 1, 1)) and v.scale() == 2.0
    for bad in (dict(delta=0.0), dict(temperatures=()), dict(temperatures=[1.0] * 9), dict(temperatures=(-1.0,)), dict(nu_cut=-1.0), dict(batch_size=0),
                dict(supercell=(1, 1)), dict(supercell=(1, 0, 1)), dict(det_min=float("nan"))):
        with pytest.raises(ValueError):
            Vibrations(pred, "energy", **bad)
    with pytest.raises(ValueError):
        Vibrations(pred, "gap")
    with pytest.raises(ValueError):
        Vibrations(SimpleNamespace(names=["energy"], hparams=dict(edge_style="knn")), "energy")


def test_dropin_config():
    text = open(os.path.join(ROOT, "dropin", "configs", "reward", "heat_capacity.yaml")).read()
    assert "_target_: rewards.calculators.HeatCapacity" in text and "_target_: rewards.reward.Reward" in text and "temperature: 300.0" in text
    assert "HeatCapacity" in open(os.path.join(ROOT, "dropin", "rewards", "calculators", "__init__.py")).read()
