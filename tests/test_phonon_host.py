"""CPU checks of the q-mesh phonons that need no GPU (matinvent_amd.phonons, include/matinvent_hip_phonon.h, matinvent_amd/csrc/phonon_fc.h;
DESIGN 51): the header, its table and the build list; the numpy restatement tests/phonon_ref64.py against the folding identity (the mesh
of a supercell's commensurate q-points holds the spectrum of the supercell's own Hessian) and against closed-form dispersions at
q-points that are not commensurate; the diagnostics and limits; the automatic supercell and its refusal; the reward calculator with the
device call replaced; and the kernels' text run on the host under the host sanitizers and held to the restatement bit for bit.  The case
lists of tests/test_gpu_phonon.py live here."""
import ctypes as C
import os
import shutil
import subprocess
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

from matinvent_amd import _lib
from tests import phonon_ref64 as R
from tests import vib_ref64 as V
from tests.header_util import ROOT, declared_symbols
from tests.test_vib_host import CV_RTOL, EIGVALSH_BOUND

# the parameters of every synthetic case, here and in tests/test_gpu_phonon.py
H, TEMPS, NU_CUT, TIE_TOL, DET_MIN = 0.01, (300.0, 10.0, 1000.0), 0.05, 1e-5, 1e-3
KERNEL_CASES = ((1, (1, 1, 1)), (1, (2, 1, 1)), (2, (2, 2, 2)), (3, (3, 1, 2)), (20, (2, 1, 1)), (22, (1, 1, 1)))   # orders 6 .. 120 (LDS), 132 (global)
# Gamma, a zone-boundary point, a point with irrational components, and the (2, 1, 1) mesh (Gamma and (1/2, 0, 0)); integer weights
Q_LIST = np.array([[0.0, 0.0, 0.0], [0.5, 0.5, 0.0], [0.5 / np.sqrt(2.0), 1.0 / np.pi, np.sqrt(3.0) / 5.0], [0.0, 0.0, 0.0], [0.5, 0.0, 0.0]])
Q_WEIGHTS = np.array([1, 2, 2, 1, 1], np.int32)
GRID_Q = Q_LIST[[0, 2]]
GRID_WEIGHTS = np.array([1, 2], np.int32)

# herm and pair_gap: the issue's bound, 6 n 2^-52, per fixture
DIAG_BOUND = lambda n: 6 * n * 2.0 ** -52


@lru_cache(maxsize=None)
def kernel_models():
    """One model per (n, reps) of KERNEL_CASES; the small ones couple every pair (range beyond half the supercell: tied images)."""
    return [R.make_model(n, reps, 300 + 7 * n + sum(reps), density=1.0 if n <= 3 else 0.3) for n, reps in KERNEL_CASES]


@lru_cache(maxsize=None)
def grid_models():
    return [R.make_model(1 + k % 3, (2, 1, 1), 2000 + k, density=1.0 if k % 2 else 0.5) for k in range(300)]


@lru_cache(maxsize=None)
def model_rows(kind, k):
    """The rows Gc of kernel model k or grid model k: computed once, shared, left unchanged."""
    md = (kernel_models() if kind == "kernel" else grid_models())[k]
    Gc = R.model_gc(md, H, seed=k)
    Gc.setflags(write=False)
    return Gc


@lru_cache(maxsize=None)
def reference(kind, k):
    """The restatement of kernel model k (on Q_LIST) or grid model k (on GRID_Q): computed once, shared, left unchanged."""
    md = (kernel_models() if kind == "kernel" else grid_models())[k]
    q, w = (Q_LIST, Q_WEIGHTS) if kind == "kernel" else (GRID_Q, GRID_WEIGHTS)
    return R.analyze(md, model_rows(kind, k), q, w, TEMPS, NU_CUT, H, TIE_TOL, DET_MIN)


def test_header_table_and_build_list():
    from matinvent_amd.build import SOURCES
    names = sorted(declared_symbols("matinvent_hip_phonon.h"))
    assert names == ["mi_phonon_dynmat", "mi_phonon_fc", "mi_phonon_thermo", "mi_phonon_workspace"]
    assert sorted(_lib.PHONON_SIGNATURES) == names and any(t is _lib.PHONON_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    assert "phonon.hip" in SOURCES
    head = open(os.path.join(ROOT, "include", "matinvent_hip_phonon.h")).read()
    fc = open(os.path.join(ROOT, "matinvent_amd", "csrc", "phonon_fc.h")).read()
    unit = open(os.path.join(ROOT, "matinvent_amd", "csrc", "phonon.hip")).read()
    assert '#include "matinvent_hip_vib.h"' in head and "fp contract(off)" in fc and "__host__ __device__" in fc and '#include "phonon_fc.h"' in unit
    assert '#include "vib_dynmat.h"' in fc
    for word in ("sin(", "cos(", "exp(", "sincos", "atomic", "mfma"):   # no transcendental function in front of the eigenvalues, no atomics, no matrix pipe
        assert word not in fc and word not in unit.split("namespace mi {", 1)[1], word
    assert "#define MI_PHONON_MAX_PRIM 128" in head and "#define MI_PHONON_IMAGES 27" in head and "PH_MAX_PRIM = 128, PH_IMAGES = 27" in fc
    assert (_lib.PHONON_MAX_PRIM, _lib.PHONON_IMAGES) == (R.MAX_PRIM, R.IMAGES) == (128, 27) and 6 * R.MAX_PRIM <= _lib.EIG_MAX_M
    assert os.path.exists(os.path.join(ROOT, "scripts", "phonon_host_check.cpp"))
    # the argument blocks are the header's structs, field for field
    for cls, struct in ((_lib.PhononFcArgs, "mi_phonon_fc_args"), (_lib.PhononDynmatArgs, "mi_phonon_dynmat_args"), (_lib.PhononThermoArgs, "mi_phonon_thermo_args")):
        body = head[head.index(f"typedef struct {struct}"):head.index(f"}} {struct};")]
        at = -1
        for k, _ in cls._fields_:
            hits = [i for i in (body.find(f" {k};", at + 1), body.find(f"*{k};", at + 1), body.find(f" {k},", at + 1), body.find(f" {k}[", at + 1)) if i >= 0]
            assert hits and min(hits) > at, (struct, k)
            at = min(hits)
    # the entries bind, and their host-only refusals answer without a GPU, by name
    lib = _lib.load()
    from matinvent_amd.phonons import ws_layout
    nbytes, off = ws_layout([2, 4, 16], (2, 1, 1))
    per = lambda n, Ns: 27 * n * Ns + (n * Ns + 1) // 2
    assert off.tolist() == [0, per(1, 2), per(1, 2) + per(2, 4), per(1, 2) + per(2, 4) + per(8, 16)] and nbytes == 8 * off[-1]
    ints = lambda *v: (C.c_int * len(v))(*v)
    assert lib.mi_phonon_workspace(ints(3), ints(2, 1, 1), 1, None) == _lib.MI_EINVAL and b"reps does not divide the atom count" in lib.mi_last_error()
    assert lib.mi_phonon_workspace(ints(129), ints(1, 1, 1), 1, None) == _lib.MI_EINVAL and b"6 n > MI_EIG_MAX_M" in lib.mi_last_error()
    assert lib.mi_phonon_workspace(ints(257), ints(1, 1, 1), 1, None) == _lib.MI_EINVAL and b"257 atoms" in lib.mi_last_error()
    assert lib.mi_phonon_workspace(ints(4), ints(2, 0, 1), 1, None) == _lib.MI_EINVAL and b"reps" in lib.mi_last_error()
    for fn in (lib.mi_phonon_fc, lib.mi_phonon_dynmat, lib.mi_phonon_thermo):
        assert fn(None, None) == _lib.MI_EINVAL and b"null argument block" in lib.mi_last_error()
    a = _lib.PhononDynmatArgs()
    a.reps, a.B, a.Q, a.T, a.table_len = ints(2, 1, 1), 1, 3, 3, 3 * 24 - 1
    assert lib.mi_phonon_dynmat(C.byref(a), None) == _lib.MI_EINVAL and b"the q-table has 71 doubles" in lib.mi_last_error()
    a.table_len = 3 * 24
    assert lib.mi_phonon_dynmat(C.byref(a), None) == _lib.MI_EINVAL and b"null pointer" in lib.mi_last_error()
    f = _lib.PhononFcArgs()
    f.h, f.det_min, f.tie_tol, f.reps, f.B, f.max_atoms = 0.01, 1e-3, -1.0, ints(1, 1, 1), 1, 4
    assert lib.mi_phonon_fc(C.byref(f), None) == _lib.MI_EINVAL and b"tie_tol" in lib.mi_last_error()


def _mesh_spectrum(md, Gc, mesh):
    """(the weighted multiset of lambda over the mesh, ascending; the processed Phi; the analysis)."""
    qp = R.mesh_points(mesh)
    res = R.analyze(md, Gc, qp, qp.weights, (300.0,), NU_CUT, H, TIE_TOL, DET_MIN)
    assert res["status"] == R.OK
    return np.sort(np.concatenate([np.repeat(res["lam"][q], int(qp.weights[q])) for q in range(len(qp.weights))])), res["Phi"], res


@pytest.mark.parametrize("n,reps,density", [(1, (2, 1, 1), 1.0), (2, (2, 1, 1), 0.5), (3, (2, 1, 1), 1.0), (1, (3, 1, 2), 1.0), (2, (3, 1, 2), 0.6), (3, (3, 1, 2), 0.4),
                                            (1, (2, 2, 2), 0.7), (2, (2, 2, 2), 1.0), (3, (2, 2, 2), 0.5)])
def test_folding_identity(n, reps, density):
    """For mesh = reps the weighted multiset of lambda over the mesh equals eigvalsh of the full 3 N_s mass-weighted supercell Hessian
    built from the same Phi, to the project's standing eigenvalue bound 4.8 M 2^-53 |A|_2 with M = 6 n.  density = 1 couples every pair
    of the supercell: the range exceeds half the supercell and the wrap-around images of a doubled axis tie (multiplicity > 1)."""
    md = R.make_model(n, reps, 40 + 11 * n + sum(reps), density=density)
    lam, Phi, res = _mesh_spectrum(md, R.model_gc(md, H, seed=n), reps)
    if density == 1.0 and 2 in reps:
        assert max(bin(int(v)).count("1") for v in res["masks"].reshape(-1)) >= 2   # tied wrap-around images
    Ds = R.supercell_dynmat(Phi, md["mass"], reps)
    assert np.array_equal(Ds, Ds.T)
    want = np.linalg.eigvalsh(Ds)
    tol = EIGVALSH_BOUND * 6 * n * 2.0 ** -53 * np.linalg.norm(Ds, 2)
    assert lam.shape == want.shape and np.abs(lam - want).max() <= tol, (np.abs(lam - want).max(), tol)


def _exact_rows(md, h):
    """Gc = +-h Phi in float64 (h a power of two: the central difference returns Phi exactly)."""
    Gc = np.empty((6 * md["n"], 3 * md["Ns"]))
    Gc[0::2], Gc[1::2] = h * md["Phi_true"], -h * md["Phi_true"]
    return Gc


def test_analytic_dispersion_off_the_commensurate_points():
    h = 2.0 ** -7
    qs = np.array([[0.137, 0.291, 0.412], [1.0 / np.pi, 0.5 / np.sqrt(2.0), 0.2], [0.5, 0.25, 0.0], [0.31, 0.0, 0.0]])
    # a monatomic cubic cell with isotropic nearest-neighbour blocks k I: omega^2 = (2 k / m) sum_d (1 - cos 2 pi q_d)
    k, m = 2.0, 55.845
    eye = np.eye(3) * k
    cubic = R.make_model(1, (3, 3, 3), 1, lat_p=np.eye(3) * 3.0, frac_p=np.zeros((1, 3)), mass=[m], blocks={(0, (1, 0, 0), 0): eye, (0, (0, 1, 0), 0): eye, (0, (0, 0, 1), 0): eye})
    res = R.analyze(cubic, _exact_rows(cubic, h), qs, np.ones(len(qs), np.int32), (300.0,), NU_CUT, h, TIE_TOL, DET_MIN)
    assert res["status"] == R.OK and res["asym"] == 0.0
    for q, lam, E in zip(qs, res["lam"], res["E"]):
        want = (2 * k / m) * (1 - np.cos(2 * np.pi * q)).sum()
        assert np.abs(lam - want).max() <= EIGVALSH_BOUND * 6 * 2.0 ** -53 * np.linalg.norm(E, 2), (q, lam, want)
    # a diatomic chain along a, reps (4, 1, 1): omega^2 = k (1/m1 + 1/m2) +- k sqrt((1/m1 + 1/m2)^2 - 4 sin^2(pi q) / (m1 m2))
    m1, m2 = 15.999, 55.845
    Kx = np.diag([k, 0.0, 0.0])
    chain = R.make_model(2, (4, 1, 1), 2, lat_p=np.diag([4.0, 5.0, 6.0]), frac_p=[[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]], mass=[m1, m2],
                         blocks={(0, (0, 0, 0), 1): Kx, (0, (-1, 0, 0), 1): Kx})
    res = R.analyze(chain, _exact_rows(chain, h), qs, np.ones(len(qs), np.int32), (300.0,), NU_CUT, h, TIE_TOL, DET_MIN)
    assert res["status"] == R.OK
    for q, lam, E in zip(qs, res["lam"], res["E"]):
        s, root = 1 / m1 + 1 / m2, np.sqrt((1 / m1 + 1 / m2) ** 2 - 4 * np.sin(np.pi * q[0]) ** 2 / (m1 * m2))
        want = np.sort([0.0] * 4 + [k * s - k * root, k * s + k * root])
        assert np.abs(lam - want).max() <= EIGVALSH_BOUND * 12 * 2.0 ** -53 * np.linalg.norm(E, 2), (q, lam, want)


def test_diagnostics_and_limits():
    from matinvent_amd.phonons import mesh_points, phase_table
    worst = 0.0
    for kind, count in (("kernel", len(KERNEL_CASES)), ("grid", 300)):
        for k in range(count):
            md, ref = (kernel_models() if kind == "kernel" else grid_models())[k], reference(kind, k)
            assert ref["status"] == R.OK and ref["asym"] < 1e-3, (kind, k)
            worst = max(worst, max(ref["herm"], ref["pair_gap"]) / DIAG_BOUND(md["n"]))
            assert ref["herm"] <= DIAG_BOUND(md["n"]) and ref["pair_gap"] <= DIAG_BOUND(md["n"]), (kind, k, ref["herm"], ref["pair_gap"])
    if os.environ.get("MI_TOL_REPORT"):
        print(f"TOL phonon diagnostics: the largest of herm and pair_gap is {worst:.3f} of 6 n 2^-52")
    for mesh in ((1, 1, 1), (2, 1, 1), (3, 1, 2), (4, 4, 4), (3, 3, 3), (2, 5, 4)):
        qp = mesh_points(mesh)
        assert int(qp.weights.sum()) == mesh[0] * mesh[1] * mesh[2] and set(qp.weights.tolist()) <= {1, 2} and np.array_equal(qp.q, qp.k / np.asarray(mesh, float))
        neg = (-qp.k) % np.asarray(mesh)
        assert all((tuple(a) == tuple(b)) == (w == 1) for a, b, w in zip(qp.k, neg, qp.weights))
    assert len(mesh_points((4, 4, 4)).weights) == 36
    # the table: conjugate under r -> -r bit for bit, exact at the quarter turns, the integer reduction of a mesh point
    tab = phase_table(mesh_points((4, 1, 3)), (2, 1, 3)).reshape(-1, 18, 2)
    ax = tab[:, :6]                       # axis a: r = -2 .. 3
    assert np.array_equal(ax[:, 1, 0], ax[:, 3, 0]) and np.array_equal(ax[:, 1, 1], -ax[:, 3, 1]) and np.array_equal(ax[:, 2], np.tile([1.0, 0.0], (len(ax), 1)))
    assert set(np.unique(ax).tolist()) <= {-1.0, 0.0, 1.0}
    irr = phase_table(Q_LIST, (3, 1, 2)).reshape(len(Q_LIST), 18, 2)
    assert np.abs(irr[..., 0] ** 2 + irr[..., 1] ** 2 - 1).max() < 4e-16 and np.array_equal(irr[:, 2, 1], -irr[:, 4, 1])
    # c_v -> 3 n k_B as T -> infinity, minus the excluded modes' share
    md, Gc = kernel_models()[2], model_rows("kernel", 2)
    hot = R.analyze(md, Gc, Q_LIST, Q_WEIGHTS, (1e9,), NU_CUT, H, TIE_TOL, DET_MIN)
    assert hot["n_imag"] == 0 and hot["n_zero"] == 3 * 2 and abs(hot["c_v"][0] - (3 * md["n"] - (hot["n_zero"] + hot["n_imag"]) / Q_WEIGHTS.sum())) < 1e-9
    assert hot["min_q"] in (0, 3) and abs(hot["min_freq"]) <= NU_CUT
    # N = 1 and n = 1: every D(q) is exactly zero
    one = reference("kernel", 0)
    assert all(not E.any() for E in one["E"]) and not one["lam"].any() and one["n_zero"] == 3 * int(Q_WEIGHTS.sum()) and not one["c_v"].any() and one["zpe"] == 0.0


def test_auto_supercell_and_the_refusal_above_256_atoms():
    from matinvent_amd import phonons
    from matinvent_amd.data import SimpleStructure
    from matinvent_amd.structure import lattice_matrix
    # a skewed cell: the plane spacings, not the edge lengths, decide
    L = lattice_matrix([4.0, 4.0, 6.0], [90.0, 90.0, 40.0])
    assert phonons.auto_reps(L, 10.0) == (4, 4, 2) and phonons.auto_reps(np.eye(3) * 5.0, 10.0) == (2, 2, 2) and phonons.auto_reps(np.eye(3) * 12.0, 10.0) == (1, 1, 1)
    hgt = abs(np.linalg.det(L)) / np.linalg.norm(np.cross(L[1], L[2]))
    assert abs(hgt - 4.0 * np.sin(np.radians(40.0))) < 1e-12 and np.ceil(10.0 / hgt) == 4
    assert phonons.auto_reps(np.zeros((3, 3)), 10.0) is None
    pred = SimpleNamespace(names=["energy"], hparams={}, normalizer=SimpleNamespace(std=[1.0]), P=1, device="cpu")
    p = phonons.Phonons(pred, "energy", supercell="auto")
    assert (p.supercell, p.min_length, p.mesh, p.delta, p.per_atom, p.temperatures, p.nu_cut, p.batch_size, p.tie_tol, p.det_min) == \
        ("auto", 10.0, (4, 4, 4), 0.01, True, (300.0,), 0.05, 256, 1e-5, 1e-3) and p.workspace_cap == phonons.WORKSPACE_CAP == 256 << 20
    assert phonons.Phonons(pred, "energy").supercell == (2, 2, 2)
    # 9 atoms in a 3 A cube: (4, 4, 4) images, 576 atoms: refused per record with status -1, never shrunk; nothing reaches the device
    rng = np.random.default_rng(0)
    big = SimpleStructure([3.0, 3.0, 3.0], [90.0, 90.0, 90.0], [8] * 9, rng.random((9, 3)))
    res = phonons.analyze_records(p, [big, "not a crystal"])
    assert res["status"].tolist() == [-1, -1] and res["reps"].tolist() == [[4, 4, 4], [0, 0, 0]] and np.isnan(res["c_v"]).all() and res["n_imag"].tolist() == [-1, -1]
    assert len(res["frequencies"]) == 2 and res["qpoints"].shape == (36, 3) and res["weights"].sum() == 64
    assert phonons.band_structure(p, [big], np.zeros((2, 3)))[0].shape == (2, 0)
    for bad in (dict(supercell="big"), dict(supercell=(1, 0, 1)), dict(mesh=(0, 1, 1)), dict(min_length=0.0), dict(tie_tol=-1.0), dict(delta=0.0), dict(workspace_cap=0)):
        with pytest.raises(ValueError):
            phonons.Phonons(pred, "energy", **bad)
    # the item list is cut under the cap, one item at least per range
    cuts, off = phonons.item_chunks([12, 12, 12, 18], 8 * 300, False)
    assert cuts == [(0, 2), (2, 3), (3, 4)] and off.tolist() == [0, 144, 0, 0]
    assert phonons.item_chunks([12, 12], 8 * 300, True)[0] == [(0, 1), (1, 2)] and phonons.item_chunks([], 10, False)[0] == []
    # the home atoms' copies alone, in balanced chunks: 18 copies under batch_size 7 are 3 chunks of 6, not 7 + 7 + 4
    assert [list(zip(s.tolist(), c.tolist())) for s, c in phonons.chunk_plan([1, 2], 7)] == [[(0, c) for c in range(6)], [(1, c) for c in range(6)], [(1, c) for c in range(6, 12)]]
    assert [len(s) for s, _ in phonons.chunk_plan([8] * 8, 256)] == [192, 192] and [len(s) for s, _ in phonons.chunk_plan([2, 3], 256)] == [30] and phonons.chunk_plan([], 4) == []
    assert all(len(s) <= 5 for s, _ in phonons.chunk_plan([3, 1, 2], 5)) and sum(len(s) for s, _ in phonons.chunk_plan([3, 1, 2], 5)) == 36


def test_the_reward_calculators_methods(monkeypatch, tmp_path):
    from matinvent_amd import phonons, rewards, vibrations
    pred = SimpleNamespace(names=["energy", "gap"], hparams={}, normalizer=SimpleNamespace(std=[1.0, 1.0]), P=2, device="cpu")
    calls = []

    def fake(which):
        def run(v, records):
            calls.append((which, v, list(records)))
            n = len(records)
            return dict(status=np.array([0, 1, 2, -1, 0][:n]), n_imag=np.array([0, 0, 0, -1, 2][:n]), c_v_gram=np.arange(1.0, n + 1)[:, None] * np.ones((1, 1)))
        return run

    monkeypatch.setattr(vibrations, "analyze_records", fake("gamma"))
    monkeypatch.setattr(phonons, "analyze_records", fake("mesh"))
    # method = "gamma" (and no method at all) constructs the same Vibrations as before
    for kw in (dict(), dict(method="gamma")):
        hc = rewards.HeatCapacity(predictor=pred, task="energy", temperature=250.0, supercell=(2, 1, 1), delta=0.02, **kw)
        assert type(hc.vib) is vibrations.Vibrations and hc.vib_kw == dict(delta=0.02, supercell=(2, 1, 1), per_atom=True)
        v = hc.vib
        assert (v.temperatures, v.supercell, v.delta, v.per_atom, v.p, v.nu_cut, v.batch_size, v.det_min) == ((250.0,), (2, 1, 1), 0.02, True, 0, 0.05, 256, 1e-3)
        assert np.array_equal(hc.calc((list("abcde"), None)), [1.0, np.nan, np.nan, np.nan, 5.0], equal_nan=True) and calls[-1][0] == "gamma"
    mesh = rewards.HeatCapacity(predictor=pred, task="energy", method="mesh", mesh=(3, 3, 2), supercell="auto", min_length=8.0, tie_tol=1e-4)
    v = mesh.vib
    assert type(v) is phonons.Phonons and (v.mesh, v.supercell, v.min_length, v.tie_tol, v.temperatures) == ((3, 3, 2), "auto", 8.0, 1e-4, (300.0,))
    assert np.array_equal(mesh.calc(list("abcde")), [1.0, np.nan, np.nan, np.nan, 5.0], equal_nan=True) and calls[-1][0] == "mesh" and calls[-1][1] is v
    strict = rewards.HeatCapacity(predictor=pred, task="energy", method="mesh", supercell=(2, 2, 1), require_stable=True)
    assert strict.vib.supercell == (2, 2, 1) and np.array_equal(strict.calc(list("abcde")), [1.0, np.nan, np.nan, np.nan, np.nan], equal_nan=True)
    with pytest.raises(ValueError):
        rewards.HeatCapacity(predictor=pred, task="energy", method="dos")
    rw = rewards.Reward(str(tmp_path / "rewards"), [dict(name="heat_capacity", calculator=mesh, target="ascending", minv=0.0, maxv=10.0)], 0.8)
    r, props, failed = rw.scoring(list("abcde"))
    assert r.tolist() == [0.1, 0.0, 0.0, 0.0, 0.5] and failed.tolist() == [False, True, True, True, False]


def test_dropin_config():
    text = open(os.path.join(ROOT, "dropin", "configs", "reward", "heat_capacity_mesh.yaml")).read()
    assert "_target_: rewards.calculators.HeatCapacity" in text and "_target_: rewards.reward.Reward" in text and "temperature: 300.0" in text
    assert "method: mesh" in text and "mesh: [4, 4, 4]" in text and "min_length: 10.0" in text and "supercell: auto" in text
    assert "method" not in open(os.path.join(ROOT, "dropin", "configs", "reward", "heat_capacity.yaml")).read()


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("phonon") / "phonon_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "phonon_host_check.cpp"), "-o", exe], check=True)
    return exe


def host_check_cases():
    """The GPU test's fixtures: the kernel models on Q_LIST, a slice of the grid on GRID_Q, then a NaN gradient element, a flat cell and
    a supercell that reps does not divide: (models, rows, reps, q, weights, references)."""
    models = list(kernel_models()) + list(grid_models()[:30])
    rows = [model_rows("kernel", k) for k in range(len(KERNEL_CASES))] + [model_rows("grid", k) for k in range(30)]
    qs = [(Q_LIST, Q_WEIGHTS)] * len(KERNEL_CASES) + [(GRID_Q, GRID_WEIGHTS)] * 30
    refs = [reference("kernel", k) for k in range(len(KERNEL_CASES))] + [reference("grid", k) for k in range(30)]
    spoiled = model_rows("kernel", 2).copy()
    spoiled[5, 7] = np.nan
    flat = dict(kernel_models()[1], lat=np.zeros((3, 3), np.float32))
    odd = dict(kernel_models()[3], reps=(2, 2, 1))   # 18 atoms, 4 images: reps does not divide the atom count
    for md, Gc in ((kernel_models()[2], spoiled), (flat, model_rows("kernel", 1)), (odd, np.zeros((0, 0)))):
        models.append(md), rows.append(Gc), qs.append((GRID_Q, GRID_WEIGHTS))
        refs.append(R.analyze(md, Gc, GRID_Q, GRID_WEIGHTS, TEMPS, NU_CUT, H, TIE_TOL, DET_MIN))
    return models, rows, [md["reps"] for md in models], qs, refs


def compare(ref, got, n, what):
    """Every output of one crystal against the restatement: equality, c_v alone to CV_RTOL (expm1)."""
    same = lambda a, b: np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    assert int(got["fc_status"]) == ref["fc_status"] and int(got["status"]) == ref["status"], (what, got["fc_status"], got["status"], ref["status"])
    if n:
        for k in ("Phi", "masks"):
            assert same(ref[k], got[k]), (what, k)
    for k in ("asym", "lam", "freqs", "zpe", "min_freq", "herm", "pair_gap", "herm_item"):
        assert same(ref[k], got[k]), (what, k, ref[k], got[k])
    for q in range(len(ref["E"])):
        assert same(ref["E"][q], got["E"][q]) and same(ref["evals"][q], got["evals"][q]), (what, q)
        assert (ref["sweeps"][q], ref["eig_status"][q]) == (int(got["sweeps"][q]), int(got["eig_status"][q])), (what, q)
    assert (ref["n_imag"], ref["n_zero"], ref["min_q"], ref["sweeps_max"]) == tuple(int(got[k]) for k in ("n_imag", "n_zero", "min_q", "sweeps_max")), what
    assert same(np.isnan(ref["c_v"]), np.isnan(got["c_v"])) and not (np.abs(ref["c_v"] - got["c_v"]) > CV_RTOL * ref["c_v"]).any(), (what, ref["c_v"], got["c_v"])   # (expm1)
    if ref["status"] != R.OK:
        assert np.isnan(got["c_v"]).all() and np.isnan(got["zpe"]) and np.isnan(got["freqs"]).all() and int(got["n_imag"]) == int(got["n_zero"]) == -1, what


def test_host_check_under_the_host_sanitizers(host_check, tmp_path):
    """scripts/phonon_host_check.cpp: the headers in the kernels' order, built with AddressSanitizer and UndefinedBehaviorSanitizer as a
    stand-alone program -- equal to the restatement in every output, bit for bit (c_v to CV_RTOL: expm1), on the fixtures of
    tests/test_gpu_phonon.py, with a NaN gradient element, with a flat cell and with a supercell that reps does not divide."""
    from matinvent_amd.phonons import phase_table
    models, rows, reps, qs, refs = host_check_cases()
    cf, of = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    R.write_case(cf, models, rows, reps, [phase_table(q, r) for (q, _), r in zip(qs, reps)], [w for _, w in qs], H, TIE_TOL, DET_MIN, NU_CUT, TEMPS)
    r = subprocess.run([host_check, cf, of], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    prim = [md["Ns"] // int(np.prod(rp)) if md["Ns"] % int(np.prod(rp)) == 0 else 0 for md, rp in zip(models, reps)]
    got = R.read_out(of, [(n, md["Ns"], len(w)) for n, md, (_, w) in zip(prim, models, qs)], len(TEMPS))
    for b, (ref, o, n) in enumerate(zip(refs, got, prim)):
        compare(ref, o, n, b)
    assert [o["status"] for o in got[-3:]] == [R.BAD_INPUT] * 3 and prim[-1] == 0 and np.isnan(got[-3]["Phi"]).all() and not got[-2]["masks"].any()
    assert sum(o["status"] != R.OK for o in got) == 3 and f"{len(models)} crystals" in r.stdout and "3 not OK" in r.stdout
