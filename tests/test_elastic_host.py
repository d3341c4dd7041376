"""CPU checks of the elasticity extension that need no GPU (matinvent_amd.elasticity, include/matinvent_hip_elastic.h,
matinvent_amd/csrc/elastic_fit.h): the header, its table and the build list; the numpy restatement tests/elastic_ref64.py
against the analytic stress derivative of the synthetic spring energy and against closed forms; the kernels' text run on the host under the
host sanitizers and held to the restatement bit for bit; the case lists of tests/test_gpu_elastic.py; the chunk plan, the reward
calculator with the device call replaced, and the drop-in configs."""
import ctypes as C
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest

from matinvent_amd import _lib
from tests import elastic_ref64 as R
from tests.header_util import ROOT, declared_symbols
from tests.test_vib_host import EIGVALSH_BOUND

# the parameters of every synthetic case, here and in tests/test_gpu_elastic.py
H, SCALE, PER_ATOM, DET_MIN = 0.005, 1.5, True, 1e-3
ATOM_COUNTS = (1, 2, 171, 20, 3)


@lru_cache(maxsize=None)
def kernel_crystals():
    return [R.make_springs(n, 100 + n) for n in ATOM_COUNTS]


@lru_cache(maxsize=None)
def grid_crystals():
    return [R.make_springs(1 + k % 3, 1000 + k) for k in range(300)]


def rows_for(Cm, h, stress0=None):
    """Workspace rows whose central difference is C (to rounding): sigma(+-j) = +-h C[:, j] / GPa, V' = 1, no flag."""
    rows = np.zeros((R.COPIES, R.ROW))
    rows[:, 6] = 1.0
    for j in range(6):
        rows[2 * j, :6] = h * np.asarray(Cm)[:, j] / R.GPA
        rows[2 * j + 1, :6] = -rows[2 * j, :6]
    if stress0 is not None:
        rows[12, :6] = stress0
    return rows


def cubic(c11, c12, c44):
    Cm = np.zeros((6, 6))
    Cm[:3, :3] = c12
    Cm[np.arange(3), np.arange(3)] = c11
    Cm[np.arange(3, 6), np.arange(3, 6)] = c44
    return Cm


def test_header_table_and_build_list():
    from matinvent_amd.build import SOURCES
    names = sorted(declared_symbols("matinvent_hip_elastic.h"))
    assert names == ["mi_elastic_collect", "mi_elastic_fit", "mi_elastic_run_chunk", "mi_elastic_strain"]
    assert sorted(_lib.ELASTIC_SIGNATURES) == names
    tables = _lib.EXTENSION_SIGNATURES
    assert tables[-1] is _lib.PRETRAIN_SIGNATURES and tables[-2] is _lib.ELASTIC_SIGNATURES and tables[-3] is _lib.VIB_SIGNATURES
    assert "elastic.hip" in SOURCES
    head = open(os.path.join(ROOT, "include", "matinvent_hip_elastic.h")).read()
    fit = open(os.path.join(ROOT, "matinvent_amd", "csrc", "elastic_fit.h")).read()
    unit = open(os.path.join(ROOT, "matinvent_amd", "csrc", "elastic.hip")).read()
    assert '#include "matinvent_hip_vib.h"' in head and "fp contract(off)" in fit and '#include "elastic_fit.h"' in unit
    assert "__host__ __device__" in fit and "not the second derivative of the energy" in head
    for k, name in enumerate(("OK", "BAD_INPUT", "SINGULAR")):
        assert f"#define MI_ELASTIC_{name} {k}" in head and f"ELASTIC_{name} = {k}" in fit
    assert (_lib.ELASTIC_OK, _lib.ELASTIC_BAD_INPUT, _lib.ELASTIC_SINGULAR) == (R.OK, R.BAD_INPUT, R.SINGULAR) == (0, 1, 2)
    assert "#define MI_ELASTIC_COPIES 13" in head and "#define MI_ELASTIC_ROW 8" in head and "ELASTIC_COPIES = 13, ELASTIC_ROW = 8" in fit
    assert (_lib.ELASTIC_COPIES, _lib.ELASTIC_ROW) == (R.COPIES, R.ROW) == (13, 8)
    assert (R.RELAX_CONVERGED, R.RELAX_FAILED, R.RELAX_EXHAUSTED) == (_lib.RELAX_CONVERGED, _lib.RELAX_FAILED, _lib.RELAX_EXHAUSTED)
    # 1 eV / A^3 in GPa from the SI value of e (exact since 2019; CODATA 2018)
    assert "ELASTIC_GPA = 160.2176634" in fit and "160.2176634" in head and R.GPA == 160.2176634
    assert abs(1.602176634e-19 / 1e-30 / 1e9 / R.GPA - 1) < 1e-15
    assert os.path.exists(os.path.join(ROOT, "scripts", "elastic_host_check.cpp"))
    # the argument blocks are the header's structs, field for field
    for cls, struct in ((_lib.ElasticChunkArgs, "mi_elastic_chunk_args"), (_lib.ElasticFitArgs, "mi_elastic_fit_args")):
        body = head[head.index(f"typedef struct {struct}"):head.index(f"}} {struct};")]
        at = -1
        for k, _ in cls._fields_:
            hits = [i for i in (body.find(f" {k};", at + 1), body.find(f"*{k};", at + 1), body.find(f" {k},", at + 1), body.find(f" {k}[", at + 1)) if i >= 0]
            assert hits and min(hits) > at, (struct, k)
            at = min(hits)
    # the entries bind, and their host-only refusals answer without a GPU
    lib = _lib.load()
    assert lib.mi_elastic_fit(None, None) == _lib.MI_EINVAL and b"null argument block" in lib.mi_last_error()
    for fn in (lib.mi_elastic_strain, lib.mi_elastic_collect):
        assert fn(None, None, None) == _lib.MI_EINVAL and b"null handle" in lib.mi_last_error()
    assert lib.mi_elastic_run_chunk(None, None, None, None, 0, None, None, None, 1, 0, None, None, None, None, None) == _lib.MI_EINVAL
    assert b"mi_elastic_run_chunk: null network" in lib.mi_last_error()
    a = _lib.ElasticFitArgs(*([None] * 13), 0.0, 1)
    assert lib.mi_elastic_fit(C.byref(a), None) == _lib.MI_EINVAL and b"finite and positive" in lib.mi_last_error()
    a = _lib.ElasticFitArgs(*([None] * 13), float("nan"), 1)
    assert lib.mi_elastic_fit(C.byref(a), None) == _lib.MI_EINVAL and b"finite and positive" in lib.mi_last_error()
    a = _lib.ElasticFitArgs(*([None] * 13), H, -1)
    assert lib.mi_elastic_fit(C.byref(a), None) == _lib.MI_EINVAL and b"B = -1" in lib.mi_last_error()
    a = _lib.ElasticFitArgs(*([None] * 13), H, 0)
    assert lib.mi_elastic_fit(C.byref(a), None) == 0   # B = 0: nothing is launched
    a = _lib.ElasticFitArgs(*([None] * 13), H, 1)
    assert lib.mi_elastic_fit(C.byref(a), None) == _lib.MI_EINVAL and b"null pointer" in lib.mi_last_error()


def test_the_strained_lattices():
    """L (I + eps) element by element: the axial copies scale one column, the shear copies mix two with h / 2 (engineering strain h), copy
    12 and a bad lattice keep their bits; and the copies of the header's plan are symmetric strains."""
    sp = kernel_crystals()[1]
    L = sp["lat"].astype(np.float64)
    for c in range(R.COPIES):
        F = R.strain_matrix(c, H)
        assert np.array_equal(F, F.T)
        want = (L @ F).astype(np.float32)
        got = R.strain(sp["lat"], c, H)
        assert got.dtype == np.float32 and np.abs(got.astype(np.float64) - L @ F).max() <= 2.0 ** -24 * np.abs(L @ F).max()
        assert np.abs(got - want).max() <= 2.0 ** -23 * np.abs(want).max()   # (L @ F sums three terms, the header two: one float32 place at most)
        if c < 12:
            a, b = R.VOIGT_AXES[c >> 1]
            hs = -H if c & 1 else H
            assert (F[a, b] + F[b, a] == hs) if a != b else (F[a, a] == 1.0 + hs)   # the Voigt (engineering) strain
            untouched = [q for q in range(3) if q not in (a, b)]
            assert np.array_equal(got[:, untouched], sp["lat"][:, untouched])
    assert np.array_equal(R.strain(sp["lat"], 12, H), sp["lat"])
    flat = np.zeros((3, 3), np.float32)
    bad = sp["lat"].copy()
    bad[1, 1] = np.inf
    for lat in (flat, bad):
        assert all(np.array_equal(R.strain(lat, c, H), lat) for c in range(R.COPIES))


def test_restatement_against_the_analytic_stress_derivative():
    """The spring energy's Cauchy stress under t E_j is a ratio of polynomials, so the exact central difference is known in closed form:
    a1 + a3 h^2 / (1 - r h^2) with a1 the analytic clamped-ion derivative (elastic_ref64.spring_stress_series).  On lattices whose strained
    copies are exact in float32 (multiples of 2^-6, h = 2^-5 and 2^-6) the restatement's raw C differs from that closed form only by
    rounding: the float32 cast of the fed gradient, |dG| <= 2^-24 |G| (half an ulp of the float32 spacing 2^-23 |G|), which reaches sigma_i
    as 2^-24 (|L'|^T |G'|)_i / V' in each of the two copies and C as their sum / (2 h); the float64 operations behind it (some twenty,
    2^-53 each) are 2^-29 of that and are covered by the factor 1.01.  So: |C_raw - exact(h)| <= that bound, the truncation error
    |C_raw - a1| is a3 h^2 / (1 - r h^2) within the same bound, and it falls by 4 (1 - r h^2 / 4) / (1 - r h^2) -- about 4 -- when h is
    halved."""
    for n, seed in ((2, 11), (3, 12), (5, 13)):
        sp = R.make_springs(n, seed, grid=True)
        s = SCALE * n
        series = [R.spring_stress_series(sp, j, s) for j in range(6)]
        a1 = np.stack([t[0] for t in series], axis=1) * R.GPA
        err = {}
        for h in (2.0 ** -5, 2.0 ** -6):
            res = R.analyze(sp, h, SCALE, PER_ATOM)
            for c in range(12):   # the strained copies are exact
                assert np.array_equal(res["lats"][c].astype(np.float64), sp["lat"].astype(np.float64) @ R.strain_matrix(c, h))
            exact = np.stack([t[0] + t[1] * h * h / (1.0 - t[2] * h * h) for t in series], axis=1) * R.GPA
            noise = np.zeros((6, 6))
            for c in range(12):
                L = np.abs(res["lats"][c].astype(np.float64))
                G = np.abs(R.spring_lattice_gradient(sp, res["lats"][c])[1]) * s
                T = L.T @ G
                noise[:, c >> 1] += 2.0 ** -24 * np.array([(T[a, b] + T[b, a]) * 0.5 for a, b in R.VOIGT_AXES]) / res["rows"][c, 6]
            noise = 1.01 * noise / (2.0 * h) * R.GPA
            assert (np.abs(res["C_raw"] - exact) <= noise).all(), (n, h, np.abs(res["C_raw"] - exact).max(), noise.max())
            trunc = np.abs(exact - a1)
            assert (np.abs(np.abs(res["C_raw"] - a1) - trunc) <= noise).all()
            err[h] = np.abs(res["C_raw"] - a1).max()
            assert res["status"] == R.OK and np.array_equal(res["C"], (res["C_raw"] + res["C_raw"].T) * 0.5) and res["n_unrelaxed"] == 0
            assert res["asym_C"] == np.abs(res["C_raw"] - res["C_raw"].T).max() / np.abs(res["C_raw"]).max()
            assert np.array_equal(res["stress0"], res["rows"][12, :6] * R.GPA) and abs(res["pressure"] + res["stress0"][:3].sum() / 3) <= 1e-15 * np.abs(res["stress0"]).max()
        ratio = err[2.0 ** -5] / err[2.0 ** -6]
        assert 3.9 < ratio < 4.1, (n, ratio, err)
        assert err[2.0 ** -6] > 100 * noise.max()   # (the truncation error is what was measured, not the rounding)


def test_isotropic_and_cubic_closed_forms():
    lam, mu = 57.0, 31.0
    res = R.fit(rows_for(cubic(lam + 2 * mu, lam, mu), H), 0.0, H)
    assert res["status"] == R.OK and res["n_negative"] == 0 and res["asym_C"] < 1e-15
    K, G = lam + 2 * mu / 3, mu
    want = [K, G, 9 * K * G / (3 * K + G), lam / (2 * (lam + mu)), K / G]
    for row in res["moduli"]:   # Voigt = Reuss = Hill
        assert np.allclose(row, want, rtol=1e-13, atol=0)
    assert np.allclose(res["moduli"][:, 2], mu * (3 * lam + 2 * mu) / (lam + mu), rtol=1e-13) and np.allclose(res["S"] @ res["C"], np.eye(6), atol=1e-14)
    assert np.allclose(res["evals"], sorted([2 * mu] * 2 + [mu] * 3 + [3 * lam + 2 * mu]), rtol=1e-13) and abs(res["cond"] - (3 * lam + 2 * mu) / mu) < 1e-12
    c11, c12, c44 = 165.0, 64.0, 79.0   # a cubic crystal
    res = R.fit(rows_for(cubic(c11, c12, c44), H, stress0=[0.01, 0.02, 0.03, 0.0, 0.0, 0.0]), 0.25, H)
    m = res["moduli"]
    gv, gr = (c11 - c12 + 3 * c44) / 5, 5 * (c11 - c12) * c44 / (4 * c44 + 3 * (c11 - c12))
    assert np.allclose(m[:, 0], (c11 + 2 * c12) / 3, rtol=1e-13) and abs(m[0, 1] / gv - 1) < 1e-13 and abs(m[1, 1] / gr - 1) < 1e-13
    assert abs(m[2, 1] / ((gv + gr) / 2) - 1) < 1e-13 and m[1, 1] < m[2, 1] < m[0, 1]
    assert np.allclose(res["stress0"], np.array([0.01, 0.02, 0.03, 0, 0, 0]) * R.GPA, rtol=1e-15) and abs(res["pressure"] + 0.02 * R.GPA) < 1e-14 and res["asym"] == 0.25


def test_indefinite_zero_and_bad_tensors():
    rng = np.random.default_rng(4)
    q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    Cm = q @ np.diag([-30.0, -2.0, 5.0, 40.0, 90.0, 200.0]) @ q.T
    res = R.fit(rows_for((Cm + Cm.T) / 2, H), 0.0, H)
    assert res["status"] == R.OK and res["n_negative"] == 2 and abs(res["cond"] - 100.0) < 1e-9 and np.isfinite(res["moduli"]).all()
    zero = R.fit(rows_for(np.zeros((6, 6)), H), 0.0, H)
    assert zero["status"] == R.SINGULAR and not zero["C"].any() and not zero["evals"].any() and np.isnan(zero["S"]).all() and zero["n_negative"] == 0
    assert zero["moduli"][0, 0] == 0.0 and zero["moduli"][0, 1] == 0.0 and np.isnan(zero["moduli"][1:]).all() and np.isnan(zero["cond"]) and zero["asym_C"] == 0.0
    rank5 = cubic(100.0, 100.0, 40.0)
    rank5[2, :3] = rank5[:3, 2] = 0.0   # an exactly zero third row and column: a zero pivot, the Voigt values kept
    one = R.fit(rows_for(rank5, H), 0.0, H)
    assert one["status"] == R.SINGULAR and np.isfinite(one["moduli"][0]).all() and np.isnan(one["moduli"][1:]).all() and np.isinf(one["cond"])
    rows = rows_for(cubic(165.0, 64.0, 79.0), H)
    rows[7, 2] = np.nan
    bad = R.fit(rows, 0.1, H)
    assert bad["status"] == R.BAD_INPUT and bad["n_negative"] == bad["n_unrelaxed"] == -1
    assert all(np.isnan(bad[k]).all() for k in ("C", "S", "stress0", "pressure", "asym", "asym_C", "moduli", "evals", "cond"))
    rows = rows_for(cubic(165.0, 64.0, 79.0), H)
    rows[[3, 12], 7] = 1.0
    assert R.fit(rows, 0.0, H)["n_unrelaxed"] == 2
    # a pivot that must be searched for: partial pivoting finds it, ties go to the lowest row
    perm = np.zeros((6, 6))
    perm[np.arange(6), [1, 0, 3, 2, 5, 4]] = 2.0
    ok, S = R.invert6(perm)
    assert ok and np.array_equal(S, perm / 4.0)


def test_jacobi_eigenvalues_against_lapack():
    """The eigenvalues of every test crystal's C (and of random symmetric 6 x 6 matrices) against numpy.linalg.eigvalsh within DESIGN 47's
    asserted bound, EIGVALSH_BOUND x M 2^-53 |A|_2."""
    mats = [R.analyze(sp, H, SCALE, PER_ATOM)["C"] for sp in kernel_crystals() + grid_crystals()[:40]]
    rng = np.random.default_rng(8)
    mats += [(a + a.T) / 2 for a in rng.standard_normal((40, 6, 6))]
    for A in mats:
        ev = R.V.jacobi(A)[0]
        assert np.abs(ev - np.linalg.eigvalsh(A)).max() <= EIGVALSH_BOUND * 6 * 2.0 ** -53 * np.linalg.norm(A, 2)


def test_chunk_plan():
    from matinvent_amd.elasticity import chunk_plan
    for B, bs in ((4, 1), (4, 5), (4, 256), (0, 5), (30, 256), (1, 13)):
        got, want = chunk_plan(B, bs), R.chunk_plan(B, bs)
        assert len(got) == len(want) == -(-13 * B // bs)
        for (s, c), w in zip(got, want):
            assert s.dtype == c.dtype == np.int32 and list(zip(s.tolist(), c.tolist())) == w and 1 <= len(w) <= bs
    flat = [p for s, c in chunk_plan(4, 5) for p in zip(s.tolist(), c.tolist())]
    assert flat == [(b, c) for b in range(4) for c in range(13)] and 13 % 5 != 0   # a crystal's copies straddle chunks


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("elastic") / "elastic_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "elastic_host_check.cpp"), "-o", exe], check=True)
    return exe


def test_host_check_under_the_host_sanitizers(host_check, tmp_path):
    """scripts/elastic_host_check.cpp: the header in the kernels' order, built with AddressSanitizer and UndefinedBehaviorSanitizer as a
    stand-alone program -- equal to the restatement in every output, bit for bit, on the crystals of tests/test_gpu_elastic.py, on a slice
    of the grid, with a NaN gradient element, a flat cell (each also in a crystal of one atom), a lattice-independent energy, and copies
    whose ion relaxation FAILED or was EXHAUSTED."""
    crystals = kernel_crystals() + grid_crystals()[:30]
    crystals = crystals + [dict(kernel_crystals()[4], lat=np.zeros((3, 3), np.float32)), dict(kernel_crystals()[0], lat=np.zeros((3, 3), np.float32)),
                           grid_crystals()[0], R.make_springs(2, 5, flat=True), kernel_crystals()[1], kernel_crystals()[3]]
    assert crystals[-4]["n"] == crystals[-5]["n"] == 1
    g = [R.spring_copies(sp, H) for sp in crystals]
    g[3] = g[3].copy()
    g[3][5, 2, 1] = np.nan
    g[-4] = g[-4].copy()
    g[-4][12, 0, 0] = np.nan
    ists = [[R.RELAX_CONVERGED] * R.COPIES for _ in crystals]
    ists[-2] = [R.RELAX_CONVERGED] * 12 + [R.RELAX_EXHAUSTED]
    ists[-2][4] = R.RELAX_EXHAUSTED
    ists[-1] = [R.RELAX_CONVERGED] * R.COPIES
    ists[-1][9] = R.RELAX_FAILED
    cf, of = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    R.write_case(cf, crystals, g, ists, H, SCALE, PER_ATOM, DET_MIN)
    r = subprocess.run([host_check, cf, of], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = R.read_out(of, len(crystals))
    same = lambda a, b: np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    for b, (sp, gg, ist, o) in enumerate(zip(crystals, g, ists, got)):
        ref = R.analyze(sp, H, SCALE, PER_ATOM, DET_MIN, g_copies=gg, ist=ist)
        for k in ("lats", "rows") + R.FIT_KEYS:
            assert same(ref[k], o[k]), (b, sp["n"], k, ref[k], o[k])
    status = [o["status"] for o in got]
    assert status[:3] == [R.OK] * 3 and status[3] == R.BAD_INPUT and status[-6:] == [R.BAD_INPUT, R.BAD_INPUT, R.BAD_INPUT, R.SINGULAR, R.OK, R.BAD_INPUT]
    assert got[-2]["n_unrelaxed"] == 2 and got[-3]["moduli"][0, 0] == 0.0 and np.isnan(got[-1]["rows"][9]).all() and np.isfinite(got[-1]["rows"][8]).all()
    assert f"{len(crystals)} crystals: {status.count(0)} ok, 5 bad input, 1 singular" in r.stdout


def test_the_reward_calculators_nan_rules(monkeypatch, tmp_path):
    from types import SimpleNamespace
    from matinvent_amd import elasticity, rewards
    pred = SimpleNamespace(names=["energy", "gap"], hparams={}, normalizer=SimpleNamespace(std=[1.0, 1.0]), P=2, device="cpu")
    calls = []

    def fake(e, records):
        calls.append((e, list(records)))
        n = len(records)
        res = elasticity.empty_results(n)
        res["status"][:] = np.array([0, 1, 2, -1, 0, 0][:n])
        res["n_negative"][:] = np.array([0, -1, 0, -1, 2, 0][:n])
        res["cond"][:] = np.array([10.0, np.nan, np.nan, np.nan, 5.0, 1e13][:n])
        res["moduli"][:] = np.arange(1.0, n + 1)[:, None, None] * np.array([1.0, 10.0, 100.0])[None, :, None] + np.arange(5)[None, None, :] * 0.1
        res["moduli"][res["status"] == 1] = np.nan
        res["moduli"][res["status"] == -1] = np.nan
        res["moduli"][res["status"] == 2, 1:] = np.nan
        return elasticity.add_shortcuts(res)

    monkeypatch.setattr(elasticity, "analyze_records", fake)
    el = rewards.Elastic(predictor=pred, task="energy", delta=0.01, ion_steps=2, relax=dict(fmax=0.05))
    out = el.calc((list("abcdef"), None))
    assert np.array_equal(out, [1.0, np.nan, 3.0, np.nan, 5.0, 6.0], equal_nan=True)   # Voigt: SINGULAR and a large cond keep their value
    e = calls[0][0]
    assert (e.delta, e.ion_steps, e.per_atom, e.p, e.batch_size, e.fire["fmax"], e.fire["dt"]) == (0.01, 2, True, 0, 256, 0.05, 0.1)
    hill = rewards.Elastic(predictor=pred, task="energy", quantity="shear_modulus", average="hill")
    assert np.array_equal(hill.calc(list("abcdef")), [100.1, np.nan, np.nan, np.nan, 500.1, np.nan], equal_nan=True)
    loose = rewards.Elastic(predictor=pred, task="energy", quantity="pugh_ratio", average="reuss", cond_max=1e14)
    assert np.array_equal(loose.calc(list("abcdef")), [10.4, np.nan, np.nan, np.nan, 50.4, 60.4], equal_nan=True)
    strict = rewards.Elastic(predictor=pred, task="energy", quantity="young_modulus", require_stable=True, relaxer=lambda s, p: (s[::-1], np.zeros(len(s))))
    assert np.array_equal(strict.calc(list("abcdef")), [1.2, np.nan, 3.2, np.nan, np.nan, 6.2], equal_nan=True) and calls[-1][1] == list("fedcba")
    assert el.calc([]).size == 0
    for bad in (dict(task=None), dict(task="energy", quantity="hardness"), dict(task="energy", average="mean"), dict(task="energy", model_path="x"),
                dict(task="energy", cond_max=0.0), dict(task="volume"), dict(task="energy", delta=0.0), dict(task="energy", relax=dict(dtt=1.0))):
        with pytest.raises(ValueError):
            rewards.Elastic(predictor=pred, **bad)
    # through Reward: a failed structure gets reward 0
    rw = rewards.Reward(str(tmp_path / "rewards"), [dict(name="bulk_modulus", calculator=el, target="ascending", minv=0.0, maxv=10.0)], 0.8)
    r, props, failed = rw.scoring(list("abcdef"))
    assert np.allclose(r, [0.1, 0.0, 0.3, 0.0, 0.5, 0.6]) and failed.tolist() == [False, True, False, True, False, False]
    assert "Elastic" in rewards.__doc__ and "DESIGN 48" in rewards.__doc__


def test_elasticity_refuses_bad_arguments():
    from types import SimpleNamespace
    from matinvent_amd.elasticity import Elasticity
    pred = SimpleNamespace(names=["energy"], hparams={}, normalizer=SimpleNamespace(std=[2.0]), P=1, device="cpu")
    e = Elasticity(pred, "energy")
    assert (e.delta, e.per_atom, e.ion_steps, e.batch_size, e.det_min) == (0.005, True, 0, 256, 1e-3) and e.scale() == 2.0
    rp = Elasticity(pred, "energy", relax=dict(fmax=0.02, n_min=3)).relax_params()
    assert (rp.relax_cell, rp.per_atom, rp.n_min, rp.scale) == (0, 1, 3, 2.0) and abs(rp.fmax - 0.02) < 1e-8 and abs(rp.dt - 0.1) < 1e-8   # (float32 fields)
    for bad in (dict(delta=0.0), dict(delta=float("inf")), dict(batch_size=0), dict(ion_steps=-1), dict(det_min=float("nan")), dict(relax=dict(fmax=-1.0)),
                dict(relax=dict(n_min=-1)), dict(relax=dict(steps=5))):
        with pytest.raises(ValueError):
            Elasticity(pred, "energy", **bad)
    with pytest.raises(ValueError):
        Elasticity(pred, "gap")
    with pytest.raises(ValueError):
        Elasticity(SimpleNamespace(names=["energy"], hparams=dict(edge_style="knn")), "energy")
    with pytest.raises(ValueError):
        Elasticity(SimpleNamespace(names=["energy"], hparams={}, normalizer=SimpleNamespace(std=[0.0])), "energy").scale()


def test_dropin_configs():
    """The four reward configs: the reference's target / minv / maxv for each name, this build's calculator."""
    want = dict(bulk_modulus=("300.0", "0.0", "250.0", "0.8"), shear_modulus=("200.0", "0.0", "160.0", "0.9"),
                young_modulus=("ascending", "80.0", "480.0", "0.8"), pugh_ratio=("ascending", "1.5", "10.0", "0.8"))
    for name, (target, minv, maxv, thr) in want.items():
        text = open(os.path.join(ROOT, "dropin", "configs", "reward", f"{name}.yaml")).read()
        assert "_target_: rewards.calculators.Elastic" in text and "_target_: rewards.reward.Reward" in text and f"quantity: {name}" in text
        assert f"- name: {name}" in text and "average: voigt" in text and f"reward_threshold: {thr}" in text
        lines = [ln.split("#")[0].strip() for ln in text.splitlines()]
        assert f"target: {target}" in lines and f"minv: {minv}" in lines and f"maxv: {maxv}" in lines
    assert "Elastic" in open(os.path.join(ROOT, "dropin", "rewards", "calculators", "__init__.py")).read()
