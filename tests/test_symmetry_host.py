"""CPU-only: the symmetry finder's definition in its executable form tests/sym_ref64.py -- the point-group table derived from
generators, the known crystals, the certificate from the input alone, the invariances, noise below and above the tolerance, primitive
cells of every Hermite-normal-form supercell, the operation cap -- and the kernels' order run on the host under the sanitizers
(scripts/sym_host_check.cpp), every output equal to the restatement bit for bit.  The restatement asserts that no decision of any fixture
lies within 1e-9 of the tolerance or of the determinant test."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import sm_cases as K
from tests import sm_ref64 as R
from tests import sym_cases as C
from tests import sym_ref64 as S
from tests.header_util import ROOT
from tests.test_struct_match_host import guard_batch


def info_of(F, b):
    return dict(zip(S.INFO, (int(v) for v in F["info"][b])))


def operations(F, b):
    n = min(int(F["info"][b][0]), S.MAX_OPS)
    return [(list(F["rot"][b, i]), list(F["trans"][b, i])) for i in range(n)]


def prepared_crystal(P, b):
    n0, n = int(P["offsets"][b]), int(P["info"][b][0])
    return P["lat"][b], P["types"][n0:n0 + n], P["frac"][n0:n0 + n]


def test_point_group_table_is_derived_and_equals_the_header():
    tab = S.derive_point_groups()
    assert [t[0] for t in tab] == list(S.PG_NAMES) and [t[1] for t in tab] == list(S.PG_ORDERS)
    assert sorted(set(S.PG_ORDERS)) == [1, 2, 3, 4, 6, 8, 12, 16, 24, 48]
    assert len(set(t[2] for t in tab)) == 32
    assert all(sum(h) == order for _, order, h in tab)
    src = open(os.path.join(ROOT, "matinvent_amd", "csrc", "sym_ops.h")).read()
    rows = re.findall(r"SYM_PG\((\d+), SYM_ROW\(([^)]*)\)\);\s*// (\S+)", src)
    assert [(int(i), name, tuple(int(x) for x in r.split(","))) for i, r, name in rows] == [(i + 1, t[0], t[2]) for i, t in enumerate(tab)]
    assert [S.crystal_system(i) for i in (1, 2, 3, 5, 6, 8, 9, 15, 16, 20, 21, 27, 28, 32)] == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7]


def test_known_crystals():
    known, (batch, P, tol, F, prim) = C.known_results()
    for b, (name, (_, n_ops, n_trans, pg)) in enumerate(known.items()):
        i = info_of(F, b)
        assert (i["n_ops"], i["n_trans"], S.PG_NAMES[i["pg_index"] - 1], i["status"]) == (n_ops, n_trans, pg, S.OK), (name, i)
        assert i["pg_order"] * i["n_trans"] == i["n_ops"] and sum(F["rot_hist"][b]) == i["pg_order"]
        assert i["has_inversion"] == (1 if pg in ("m-3m", "6/mmm", "4/mmm", "-1") else 0)
    systems = {name: int(F["info"][b][5]) for b, name in enumerate(known)}
    assert systems["sc"] == 7 and systems["hcp"] == 6 and systems["rutile"] == 4 and systems["triclinic"] == 1
    assert (np.asarray(F["ptrans"][list(known).index("rocksalt_conv"), 0]) == 0.0).all()


def test_certificate_of_every_returned_operation():
    """From the prepared cell and coordinates alone, with numpy's own operations: every (W, t) maps atoms onto atoms of their species
    within tol, W L keeps the lengths within tol, and the set is closed under composition whenever the status is OK."""
    known, (batch, P, tol, F, prim) = C.known_results()
    for b in range(len(known)):
        assert S.certificate(prepared_crystal(P, b), float(tol[b]), operations(F, b), complete=int(F["info"][b][7]) == S.OK)
    crystals, (batch, P, tol, F, prim) = C.random_results()
    for b in range(len(crystals)):
        assert S.certificate(prepared_crystal(P, b), float(tol[b]), operations(F, b), complete=int(F["info"][b][7]) == S.OK)


def test_invariance_under_the_transformations():
    known, (batch, P, tol, F, prim) = C.known_results()
    rng = np.random.default_rng(31)
    names = ["rocksalt_conv", "wurtzite", "rutile", "zincblende", "triclinic_inversion", "triclinic_2x1x1"]
    copies = [K.transformed(rng, known[n][0], scale=1.0) for n in names]
    _, _, _, F2, prim2 = C.analyse(copies)
    for b2, n in enumerate(names):
        b = list(known).index(n)
        for k in (0, 1, 3, 4, 5, 6, 7):   # everything but the map count of the reduced cell's metric
            assert F2["info"][b2][k] == F["info"][b][k], (n, S.INFO[k])
        assert list(F2["rot_hist"][b2]) == list(F["rot_hist"][b]), n
        assert prim2["prim_count"][b2] == prim["prim_count"][b]


def test_noise_below_the_tolerance_keeps_and_above_it_breaks():
    known, (batch, P, tol, F, prim) = C.known_results()
    rng = np.random.default_rng(41)
    names = ["rocksalt_conv", "wurtzite", "rutile", "diamond"]
    noisy = []
    for n in names:
        L, z, f = known[n][0]
        d = rng.normal(size=f.shape) * 0.15 * C.SYMPREC
        norm = np.linalg.norm(d, axis=1, keepdims=True)
        d = d * np.minimum(1.0, 0.3 * C.SYMPREC / np.maximum(norm, 1e-30))     # every atom's deviation <= 0.3 symprec
        noisy.append((L, z, f + d @ np.linalg.inv(L)))
    L, z, f = known["rocksalt_conv"][0]
    d = rng.normal(size=f.shape)
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * 5.0 * C.SYMPREC
    noisy.append((L, z, f + d @ np.linalg.inv(L)))
    _, _, _, F2, _ = C.analyse(noisy)
    for b2, n in enumerate(names):
        b = list(known).index(n)
        assert list(F2["info"][b2]) == list(F["info"][b]) and list(F2["rot_hist"][b2]) == list(F["rot_hist"][b]), n
        assert 0.0 < F2["dev"][b2, :int(F2["info"][b2][0])].max() < tol[b]   # (the translation carries two atoms' noise, the image and the target one each)
    last = info_of(F2, len(names))
    assert (last["n_ops"], last["n_trans"], last["pg_index"], last["status"]) == (1, 1, 1, S.OK)


def test_primitive_cell_of_every_supercell():
    """Every Hermite-normal-form supercell of index 2 .. 8 of a one-atom and of a three-atom triclinic crystal reduces to n / index atoms
    with |det| = 1 / index: the condition that a basis triple exists among the translations and the unit vectors."""
    rng = np.random.default_rng(53)
    bases = [K.random_crystal(rng, [1]), K.random_crystal(rng, [2, 1])]
    for base in bases:
        crystals, index = [], []
        for idx in range(2, 9):
            for H in C.hnf_matrices(idx):
                crystals.append(C.supercell(base, H))
                index.append(idx)
        batch, P, tol, F, prim = C.analyse(crystals)
        for b, idx in enumerate(index):
            assert not int(prim["prim_status"][b]) & S.PRIM_FAIL, (b, idx)
            assert int(F["info"][b][1]) == idx and int(F["info"][b][7]) & ~S.NOT_A_GROUP == S.OK, (b, idx, list(F["info"][b]))
            assert int(prim["prim_count"][b]) == len(base[1]) and abs(prim["prim_det"][b] * idx - 1.0) <= 1e-9, (b, idx)
            vol = abs(np.linalg.det(prim["lat"][b].reshape(3, 3).astype(np.float64)))
            assert abs(vol / abs(np.linalg.det(base[0])) - 1.0) < 1e-5
        assert list(prim["prim_offsets"]) == list(np.arange(len(crystals) + 1) * len(base[1]))


def test_rocksalt_reduces_to_the_fcc_cell():
    known, (batch, P, tol, F, prim) = C.known_results()
    b = list(known).index("rocksalt_conv")
    lo, hi = int(prim["prim_offsets"][b]), int(prim["prim_offsets"][b + 1])
    assert hi - lo == 2 and sorted(prim["types"][lo:hi]) == [11, 17] and prim["prim_status"][b] == S.OK
    assert abs(abs(np.linalg.det(prim["lat"][b].reshape(3, 3).astype(np.float64))) - K.A0 ** 3 / 4) < 1e-4
    d = (prim["frac"][lo] - prim["frac"][lo + 1]).astype(np.float64)
    assert np.allclose(np.abs(d - np.round(d)), 0.5, atol=1e-6)
    # crystals with one pure translation are copied bit for bit
    off = batch[0]
    for c, name in enumerate(known):
        if int(F["info"][c][1]) == 1:
            p0 = int(prim["prim_offsets"][c])
            n = int(off[c + 1] - off[c])
            assert np.array_equal(prim["frac"][p0:p0 + n], batch[2][off[c]:off[c + 1]]) and np.array_equal(prim["lat"][c], batch[3][c]), name
    # the primitive cell of the conventional cell matches the primitive cell under the restated matcher
    pc = (prim["lat"][b].reshape(3, 3), list(prim["types"][lo:hi]), prim["frac"][lo:hi])
    Q = R.prepare(*K.batch([pc, K.cell("rocksalt_prim")]))
    r = R.match_pair(Q, 0, Q, 1, 0.2, K.COS_TOL)
    assert r["status"] == R.OK and r["rms"] < 1e-5


def test_operation_cap_on_the_4x4x4_supercell():
    batch, P, tol, F, prim = C.capped_results()
    i = info_of(F, 0)
    assert (i["n_ops"], i["n_trans"], i["pg_order"], S.PG_NAMES[i["pg_index"] - 1], i["status"]) == (3072, 64, 48, "m-3m", S.OPS_CAP)
    assert int(prim["prim_count"][0]) == 1 and list(prim["prim_offsets"]) == [0, 1] and int(prim["prim_status"][0]) == S.OPS_CAP
    assert abs(prim["prim_det"][0] * 64 - 1.0) <= 1e-9
    assert S.certificate(prepared_crystal(P, 0), float(tol[0]), operations(F, 0)[::7], complete=False)


def test_statuses_of_the_guard_batch():
    off, types, frac, lat, _ = guard_batch()
    P = R.prepare(off, types, frac, lat)
    tol = S.tolerances(np.clip(off, 0, len(types)), lat, C.SYMPREC)
    F = S.find(P, tol, K.COS_TOL, fill=-7)
    ok = [b for b in range(len(lat)) if P["info"][b][3] == R.PREP_OK]
    assert ok == [0, 5, 9]
    for b in range(len(lat)):
        if b in ok:
            assert F["info"][b][7] == S.OK and F["info"][b][0] >= 1
        else:
            assert list(F["info"][b]) == [0] * 7 + [S.NOT_PREPARED] and (F["rot"][b] == -7).all() and (F["ptrans"][b] == -7).all()
    bad = S.find(P, np.where(np.arange(len(lat)) == 0, np.nan, tol), K.COS_TOL)
    assert bad["info"][0][7] == S.BAD_TOL and bad["info"][5][7] == S.OK


# ---- the kernels' order on the host, under the sanitizers ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("sym") / "sym_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "sym_host_check.cpp"), "-o", exe], check=True)
    return exe


def run_host_check(exe, tmp_path, off, types, frac, lat, tol):
    B, N = len(off) - 1, len(types)
    cf, of = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(cf, "wb") as f:
        f.write(struct.pack("<ii", B, N) + struct.pack("<d", K.COS_TOL))
        for arr, dt in ((off, np.int32), (types, np.int32), (frac, np.float32), (lat, np.float32), (tol, np.float64)):
            f.write(np.ascontiguousarray(np.asarray(arr, dt)).tobytes())
    r = subprocess.run([exe, cf, of], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(of, "rb").read()
    out, pos = {}, 0
    for name, shape, dt in (("info", (B, 8), np.int32), ("rot_hist", (B, 10), np.int32), ("rot", (B, 192, 9), np.int32), ("trans", (B, 192, 3), np.float64),
                            ("dev", (B, 192), np.float64), ("ptrans", (B, 64, 3), np.float64), ("prim_count", (B,), np.int32), ("prim_status", (B,), np.int32),
                            ("prim_det", (B,), np.float64), ("prim_offsets", (B + 1,), np.int32), ("types", (N,), np.int32), ("frac", (N, 3), np.float32),
                            ("lat", (B, 9), np.float32)):
        size = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[name] = np.frombuffer(raw[pos:pos + size], dt).reshape(shape)
        pos += size
    assert pos == len(raw)
    return out


def assert_equal_bits(got, F, prim):
    for k in ("info", "rot_hist", "rot", "trans", "dev", "ptrans"):
        assert np.array_equal(got[k], F[k]), k
    for k in ("prim_count", "prim_status", "prim_det", "prim_offsets", "types", "frac", "lat"):
        assert np.array_equal(got[k], prim[k], equal_nan=True), k


def test_host_check_equals_the_restatement(host_check, tmp_path):
    known = C.known_crystals()
    crystals = [v[0] for v in known.values()] + C.random_set()
    batch, P, tol, F, prim = C.analyse(crystals, fill=-7)
    assert_equal_bits(run_host_check(host_check, tmp_path, *batch, tol), F, prim)


def test_host_check_equals_the_restatement_on_the_guards_and_the_cap(host_check, tmp_path):
    off, types, frac, lat, _ = guard_batch()
    P = R.prepare(off, types, frac, lat)
    tol = S.tolerances(np.clip(off, 0, len(types)), lat, C.SYMPREC)
    F = S.find(P, tol, K.COS_TOL, fill=-7)
    prim = S.primitive(P, types, frac, lat, F, fill=-7)
    assert_equal_bits(run_host_check(host_check, tmp_path, off, types, frac, lat, tol), F, prim)
    batch = K.batch([C.sc_supercell_444()])
    P = R.prepare(*batch)
    _, _, tol, F0, _ = C.capped_results()
    got = run_host_check(host_check, tmp_path, *batch, tol)
    assert np.array_equal(got["info"], F0["info"]) and np.array_equal(got["rot"], F0["rot"]) and np.array_equal(got["ptrans"][0], F0["ptrans"][0])
    assert np.array_equal(got["trans"], F0["trans"]) and np.array_equal(got["dev"], F0["dev"]) and list(got["prim_offsets"]) == [0, 1]


def test_header_table_constants_and_the_drop_in():
    from matinvent_amd import _lib, rewards, symmetry
    from matinvent_amd.build import SOURCES
    from tests.header_util import declared_symbols
    names = declared_symbols("matinvent_hip_sym.h")
    assert names == ["mi_sym_find", "mi_sym_primitive"] and sorted(_lib.SYM_SIGNATURES) == names and "symmetry.hip" in SOURCES
    assert any(t is _lib.SYM_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    head = open(os.path.join(ROOT, "include", "matinvent_hip_sym.h")).read()
    ops = open(os.path.join(ROOT, "matinvent_amd", "csrc", "sym_ops.h")).read()
    for name in ("OK", "NOT_PREPARED", "BOX_CAP", "MAP_CAP", "NO_LATTICE", "AMBIGUOUS", "OPS_CAP", "NOT_A_GROUP", "PRIM_FAIL", "BAD_TOL"):
        v = getattr(S, name)
        assert f"#define MI_SYM_{name} {v}\n" in head and f"SYM_{name} = {v}" in ops and getattr(_lib, "SYM_" + name) == v, name
    assert '#include "sm_assign.h"' in ops and "fp contract(off)" in ops and "__host__ __device__" in open(os.path.join(ROOT, "matinvent_amd", "csrc", "sm_lattice.h")).read()
    assert (_lib.SYM_MAX_OPS, _lib.SYM_MAX_TRANS, _lib.SYM_INFO, _lib.SYM_CLASSES) == (S.MAX_OPS, S.MAX_TRANS, S.NINFO, S.NCLASS)
    assert symmetry.POINT_GROUPS[1:] == S.PG_NAMES and symmetry.INFO == S.INFO and symmetry.CLASSES == S.CLASSES
    known = C.known_crystals()
    off, types, frac, lat = K.batch([v[0] for v in known.values()])
    assert np.array_equal(symmetry.tolerances(np.diff(off), lat, 0.1), S.tolerances(off, lat, 0.1))
    with pytest.raises(ValueError):
        rewards.Symmetry(quantity="hall_number")
    with pytest.raises(ValueError):
        rewards.Symmetry(symprec=0.0)
    assert rewards.Symmetry("not_p1").calc([]).shape == (0,) and "Symmetry" in rewards.__doc__
    text = open(os.path.join(ROOT, "dropin", "configs", "reward", "symmetry.yaml")).read()
    assert "_target_: rewards.calculators.Symmetry" in text and "_target_: rewards.reward.Reward" in text and "symprec: 0.1" in text
    assert "Symmetry" in open(os.path.join(ROOT, "dropin", "rewards", "calculators", "__init__.py")).read()
