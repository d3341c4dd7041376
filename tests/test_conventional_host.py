"""CPU-only: the conventional cell's definition in its executable form tests/conv_ref64.py -- the 14 Bravais lattices as typed and
transformed, the known crystals, crystals of lower symmetry than their metric, the certificate recomputed from the outputs in numpy, the
round trip through the primitive cell, the margins of the search box and of its decisions, the invariance of the cell parameters, the
statuses -- and the kernels' order run on the host under the sanitizers (scripts/sym_conv_host_check.cpp), every output equal to the
restatement bit for bit."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import conv_cases as CC
from tests import conv_ref64 as V
from tests import sm_cases as K
from tests import sm_ref64 as R
from tests import sym_cases as C
from tests import sym_ref64 as S
from tests.header_util import ROOT
from tests.test_struct_match_host import guard_batch

# The largest relative deviation of a cell parameter between a fixture and its transformed copy under the restatement (lengths over the
# cube root of the volume ratio; float32 cells, unimodular coefficients up to a few units), measured at 2.24e-7 on oS_A: the bound is four
# times that.  A wrong identification shows as 1e-1.
INVARIANCE_MEASURED = 2.24e-7
INVARIANCE_BOUND = 4 * INVARIANCE_MEASURED
AMBIGUOUS_CRYSTAL = (np.eye(3) * 4.0, [29, 29], np.array([[0, 0, 0], [0.012, 0, 0]], np.float64))   # two atoms of a species 0.05 A apart


def info_of(conv, b):
    return dict(zip(V.INFO, (int(v) for v in conv["conv_info"][b])))


def primitive_of(ch, b):
    p = ch["prim"]
    lo, hi = int(p["prim_offsets"][b]), int(p["prim_offsets"][b + 1])
    return p["lat"][b].reshape(3, 3).astype(np.float64), [int(v) for v in p["types"][lo:hi]], p["frac"][lo:hi].astype(np.float64)


def test_identification_of_every_fixture():
    cases, batch, ch = CC.fixture_results()
    conv = ch["conv"]
    assert len(cases) == 2 * (17 + 6) + 13
    seen = set()
    for b, (name, _, (system, mult, letter)) in enumerate(cases):
        i = info_of(conv, b)
        assert i["status"] == S.OK and i["bravais"] >= 1, (name, i)
        assert (i["crystal_system"], i["mult"]) == (system, mult), (name, i)
        assert letter is None or V.CENTRING[i["centring"]] == letter, (name, i)
        assert i["bravais"] == V.bravais_of(system, i["centring"]) and i["max_m"] <= 2 and i["zero"] == 0, (name, i)
        assert int(conv["conv_count"][b]) == mult * int(ch["prim"]["prim_count"][b]), name
        seen.add(V.BRAVAIS[i["bravais"]])
        if V.CENTRING[i["centring"]] == "R":   # always obverse
            assert conv["conv_cvec"][b].tolist() == [[0, 0, 0], [1, 2, 2], [2, 1, 1], [0, 0, 0]], name
        if name.startswith("mS"):
            assert V.CENTRING[i["centring"]] in ("A", "C", "I") and V.BRAVAIS[i["bravais"]] == "mS", (name, i)
    assert seen == set(V.BRAVAIS[1:])   # all 14
    names = [c[0] for c in cases]
    assert [V.BRAVAIS[conv["conv_info"][names.index(n)][0]] for n in ("oS_C", "oS_A", "oS_C~", "oS_A~")] == ["oS"] * 4
    assert int(conv["conv_info"][names.index("pyrite")][4]) == 3 and S.PG_NAMES[int(ch["F2"]["info"][names.index("pyrite")][4]) - 1] == "m-3"
    assert int(conv["conv_info"][names.index("hex_metric_3m")][3]) == 5 and V.BRAVAIS[conv["conv_info"][names.index("hex_metric_3m")][0]] == "hP"


def test_certificate_recomputed_from_the_outputs():
    """|det M| = mult; mult x n_prim distinct atoms; the metric meets its system's constraints; every atom is a primitive atom plus a
    lattice vector -- in numpy's own operations, from the outputs and the primitive crystal alone."""
    cases, batch, ch = CC.fixture_results()
    conv = ch["conv"]
    for b, (name, _, _) in enumerate(cases):
        i = info_of(conv, b)
        assert V.certificate(primitive_of(ch, b), V.crystal_of(conv, b), conv["conv_M"][b], i["mult"], i["crystal_system"], i["centring"], CC.SYMPREC, CC.ANGLE_TOL), name
        params = V.cell_parameters(V.crystal_of(conv, b)[0])
        if i["crystal_system"] == 2:
            assert params[4] >= 90.0 - 1e-4, (name, params)
        if i["crystal_system"] == 3:
            assert params[0] <= params[1] * (1 + 1e-6) and (V.CENTRING[i["centring"]] == "C" or params[1] <= params[2] * (1 + 1e-6)), (name, params)


def test_conventional_structure_matches_the_input():
    """Under the restated matcher with both sides reduced to their primitive cells."""
    cases, batch, ch = CC.fixture_results()
    conv = ch["conv"]
    crystals = [V.crystal_of(conv, b) for b in range(len(cases))]
    cb = K.batch(crystals)
    Pc = R.prepare(*cb)
    Fc = S.find(Pc, S.tolerances(cb[0], cb[3], CC.SYMPREC), K.COS_TOL, margin=False)
    pc = S.primitive(Pc, cb[1], cb[2], cb[3], Fc, margin=False)
    Qc = R.prepare(pc["prim_offsets"], pc["types"], pc["frac"], pc["lat"])
    Qi = ch["P2"]
    for b, (name, _, _) in enumerate(cases):
        assert int(pc["prim_count"][b]) == int(ch["prim"]["prim_count"][b]), name
        r = R.match_pair(Qi, b, Qc, b, 0.2, K.COS_TOL)
        assert r["status"] == R.OK and r["rms"] < 1e-4, (name, r["status"], r["rms"])


def test_round_trip_of_rock_salt():
    cases, batch, ch = CC.fixture_results()
    b = [c[0] for c in cases].index("rocksalt_conv")
    assert int(ch["prim"]["prim_count"][b]) == 2 and int(ch["conv"]["conv_count"][b]) == 8 and V.BRAVAIS[ch["conv"]["conv_info"][b][0]] == "cF"
    got = V.crystal_of(ch["conv"], b)
    Q = R.prepare(*K.batch([got, K.cell("rocksalt_conv")]))
    r = R.match_pair(Q, 0, Q, 1, 0.2, K.COS_TOL)
    assert r["status"] == R.OK and r["rms"] < 1e-5
    assert np.allclose(V.cell_parameters(got[0]), [K.A0] * 3 + [90.0] * 3, rtol=INVARIANCE_BOUND)


def test_box_of_two_equals_box_of_four():
    for cases, batch, ch in (CC.fixture_results(), CC.random_results()):
        p = ch["prim"]
        wide = V.conventional(ch["P2"], p["types"], p["frac"], p["lat"], ch["F2"], box=4)
        for k in ("conv_info", "conv_M", "conv_cvec", "conv_count", "conv_offsets", "types", "frac", "lat"):
            assert np.array_equal(wide[k], ch["conv"][k]), k
        assert int(ch["conv"]["conv_info"][:, 5].max()) <= 2


def test_decisions_keep_their_margin():
    """Every search of the fixtures ran with the margin assertion on (fixture_results would have raised).  A knife edge raises: in a plane
    of hexagonal metric under a two-fold axis alone the third-shortest vector ties with the second and no operation carries one onto the
    other."""
    CC.fixture_results()
    G = [1.0, -0.5, 0.0, -0.5, 1.0, 0.0, 0.0, 0.0, 2.0]
    two_fold_sum = V.axis_sum([-1, 0, 0, 0, -1, 0, 0, 0, 1], 2)
    only_signs = lambda k: {tuple(k), tuple(-v for v in k)}
    a = V.search(two_fold_sum, None, G, V.BOX)
    assert a == [1, 1, 0]   # (of the six vectors of length 1 the lexicographically largest)
    with pytest.raises(AssertionError):
        V.search(two_fold_sum, a, G, V.BOX, only_signs)
    G[1] = G[3] = -0.3
    G[4] = 1.3   # an oblique plane: squared lengths 1, 1.3, 1.7: no tie
    a = V.search(two_fold_sum, None, G, V.BOX, only_signs)
    assert a == [1, 0, 0] and V.search(two_fold_sum, a, G, V.BOX, only_signs) == [0, 1, 0]


def invariance_deviations():
    cases, batch, ch = CC.fixture_results()
    conv, names, out = ch["conv"], [c[0] for c in cases], {}
    for b, name in enumerate(names):
        if not name.endswith("~"):
            continue
        a = names.index(name[:-1])
        La, Lb = V.crystal_of(conv, a)[0], V.crystal_of(conv, b)[0]
        s = (abs(np.linalg.det(Lb)) / abs(np.linalg.det(La))) ** (1.0 / 3.0)
        pa, pb = np.array(V.cell_parameters(La)), np.array(V.cell_parameters(Lb))
        pb[:3] /= s
        if int(conv["conv_info"][a][3]) == 1:   # triclinic: the reduced cell as it comes, which names its axes by the input's; the lengths as a set
            out[name] = float(np.abs(np.sort(pb[:3]) / np.sort(pa[:3]) - 1.0).max())
        else:
            out[name] = float(np.abs(pb / pa - 1.0).max())
    return out


def test_cell_parameters_do_not_depend_on_the_cell_given():
    dev = invariance_deviations()
    print({k: f"{v:.3e}" for k, v in dev.items()})
    assert len(dev) == 23 and INVARIANCE_BOUND < 1e-4
    assert max(dev.values()) <= INVARIANCE_BOUND, max(dev.items(), key=lambda kv: kv[1])


def status_batch():
    """Rock salt, a crystal whose analysis is ambiguous, rock salt; then the guard batch of the matcher's tests."""
    off, types, frac, lat, _ = guard_batch()
    head = K.batch([CC.rocksalt_prim(), AMBIGUOUS_CRYSTAL, CC.rocksalt_prim()])
    n = len(head[1])
    return (np.concatenate([head[0], np.asarray(off[1:], np.int64) + n]).astype(np.int32), np.concatenate([head[1], types]).astype(np.int32),
            np.concatenate([head[2], np.asarray(frac, np.float32)]), np.concatenate([head[3], np.asarray(lat, np.float32).reshape(-1, 9)]))


def test_statuses():
    batch = status_batch()
    ch = V.chain(batch, CC.SYMPREC, K.COS_TOL, fill=-7)
    conv, F2 = ch["conv"], ch["F2"]
    assert info_of(conv, 0)["bravais"] == 14 and info_of(conv, 2)["bravais"] == 14 and int(conv["conv_count"][0]) == 8
    amb = info_of(conv, 1)
    assert int(F2["info"][1][7]) & (S.AMBIGUOUS | S.NOT_A_GROUP) and amb["status"] == int(F2["info"][1][7]) | V.CONV_FAIL and amb["bravais"] == 0 and amb["mult"] == 1
    lo, hi = int(conv["conv_offsets"][1]), int(conv["conv_offsets"][2])
    p = ch["prim"]
    q0 = int(p["prim_offsets"][1])
    assert hi - lo == 2 and np.array_equal(conv["frac"][lo:hi], p["frac"][q0:q0 + 2]) and np.array_equal(conv["lat"][1], p["lat"][1])   # unchanged, bit for bit
    assert np.array_equal(conv["frac"][lo:hi], batch[2][2:4]) and np.array_equal(conv["lat"][1], batch[3][1])
    flagged = [b for b in range(len(batch[3])) if ch["P2"]["info"][b][3] != R.PREP_OK]
    assert len(flagged) == 7
    for b in flagged:
        i = info_of(conv, b)
        assert i["status"] & S.NOT_PREPARED and i["status"] & V.CONV_FAIL and i["bravais"] == 0 and int(conv["conv_count"][b]) == 0
        assert int(conv["conv_offsets"][b]) == int(conv["conv_offsets"][b + 1]) and (conv["lat"][b] == -7).all()
    total = int(conv["conv_offsets"][-1])
    assert (conv["types"][total:] == -7).all() and (conv["frac"][total:] == -7).all() and (conv["types"][:total] != -7).all()
    ok = [b for b in range(len(batch[3])) if b not in flagged and b != 1]
    assert all(info_of(conv, b)["status"] == S.OK for b in ok)


# ---- the kernels' order on the host, under the sanitizers ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("symconv") / "sym_conv_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "sym_conv_host_check.cpp"), "-o", exe], check=True)
    return exe


def run_host_check(exe, tmp_path, ch):
    P2, F2, p = ch["P2"], ch["F2"], ch["prim"]
    B, N = len(p["lat"]), len(p["types"])
    cf, of = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(cf, "wb") as f:
        f.write(struct.pack("<ii", B, N))
        for arr, dt in ((P2["offsets"], np.int32), (P2["info"], np.int32), (P2["lat"], np.float64), (p["types"], np.int32), (p["frac"], np.float32),
                        (p["lat"], np.float32), (F2["info"], np.int32), (F2["rot"], np.int32)):
            f.write(np.ascontiguousarray(np.asarray(arr, dt)).tobytes())
    r = subprocess.run([exe, cf, of], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(of, "rb").read()
    out, pos = {}, 0
    for name, shape, dt in (("conv_info", (B, 8), np.int32), ("conv_M", (B, 9), np.int32), ("conv_cvec", (B, 4, 3), np.int32), ("conv_count", (B,), np.int32),
                            ("conv_offsets", (B + 1,), np.int32), ("types", (4 * N,), np.int32), ("frac", (4 * N, 3), np.float32), ("lat", (B, 9), np.float32)):
        size = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[name] = np.frombuffer(raw[pos:pos + size], dt).reshape(shape)
        pos += size
    assert pos == len(raw)
    return out


def assert_equal_bits(got, conv):
    for k in ("conv_info", "conv_M", "conv_cvec", "conv_count", "conv_offsets", "types", "frac", "lat"):
        assert np.array_equal(got[k], conv[k], equal_nan=True), k


def test_host_check_equals_the_restatement(host_check, tmp_path):
    cases = CC.all_cases()
    batch = K.batch([c[1] for c in cases] + C.random_set())
    ch = V.chain(batch, CC.SYMPREC, K.COS_TOL, fill=-7)
    assert_equal_bits(run_host_check(host_check, tmp_path, ch), ch["conv"])


def test_host_check_equals_the_restatement_on_the_statuses(host_check, tmp_path):
    ch = V.chain(status_batch(), CC.SYMPREC, K.COS_TOL, fill=-7)
    assert_equal_bits(run_host_check(host_check, tmp_path, ch), ch["conv"])


def test_header_table_constants_and_the_consumers():
    from matinvent_amd import _lib, rewards, substrates, symmetry
    from matinvent_amd.build import ALL_SOURCES, SOURCES
    from tests.header_util import declared_symbols
    names = declared_symbols("matinvent_hip_sym_conv.h")
    assert names == ["mi_sym_conventional"] and sorted(_lib.SYM_CONV_SIGNATURES) == names
    assert "sym_conv.hip" in ALL_SOURCES and len(set(ALL_SOURCES)) == len(ALL_SOURCES) and set(SOURCES) < set(ALL_SOURCES)
    assert any(t is _lib.SYM_CONV_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    head = open(os.path.join(ROOT, "include", "matinvent_hip_sym_conv.h")).read()
    ops = open(os.path.join(ROOT, "matinvent_amd", "csrc", "sym_conv.h")).read()
    unit = open(os.path.join(ROOT, "matinvent_amd", "csrc", "sym_conv.hip")).read()
    assert "#define MI_SYM_CONV_FAIL 512\n" in head and "SYM_CONV_FAIL = 512" in ops and _lib.SYM_CONV_FAIL == V.CONV_FAIL == 512
    assert "MI_SYM_CONV_FAIL" not in open(os.path.join(ROOT, "include", "matinvent_hip_sym.h")).read()
    assert '#include "sym_ops.h"' in ops and "fp contract(off)" in ops and '#include "sym_conv.h"' in unit
    for word in ("atomic", "mfma", "sqrt", "floor("):   # no atomics, no matrix pipe; + - x / only in the new header
        assert word not in ops, word
    for word in ("atomic", "mfma"):
        assert word not in unit.split("namespace mi {", 1)[1], word
    for k, v in (("BOX", V.BOX), ("MAX_MULT", V.MAX_MULT), ("M_MAX", V.M_MAX), ("T_MAX", V.T_MAX), ("INFO", V.NINFO)):
        assert f"CONV_{k} = {v}" in ops, k
    assert f"CONV_Q_MAX = 1 << {V.Q_MAX.bit_length() - 1}" in ops and 3 * V.M_MAX * V.T_MAX < V.Q_MAX and 2 * V.Q_MAX ** 2 < 2 ** 31
    assert (_lib.SYM_CONV_INFO, _lib.SYM_CONV_MAX_MULT) == (V.NINFO, V.MAX_MULT)
    assert symmetry.BRAVAIS == V.BRAVAIS and symmetry.CENTRINGS == V.CENTRING and symmetry.CONV_INFO == V.INFO
    for letter, index in zip(("NONE", "P", "A", "B", "C", "I", "F", "R"), range(8)):
        assert f"CONV_{letter} = {index}" in ops
    for q in ("bravais", "centring_mult"):
        assert rewards.Symmetry(q).calc([]).shape == (0,)
    cell = [5.4437] * 3 + [90.0] * 3
    with pytest.raises(ValueError, match="primitive=True and conventional=True"):
        rewards.PyMatGen(task="mcia", substrate=cell, primitive=True, conventional=True)
    with pytest.raises(ValueError, match="primitive=True and conventional=True"):
        substrates.match_records(None, [], None, primitive=True, conventional=True)
    with pytest.raises(ValueError, match="primitive=True and conventional=True"):
        substrates.mcia([], cell, primitive=True, conventional=True)
    assert rewards.PyMatGen(task="mcia", substrate=cell).conventional is False and rewards.PyMatGen(task="mcia", substrate=cell, conventional=True).conventional is True
    text = open(os.path.join(ROOT, "dropin", "configs", "reward", "mcia_conventional.yaml")).read()
    assert "_target_: rewards.calculators.PyMatGen" in text and "conventional: true" in text and "task: mcia" in text
    assert "conventional:" not in open(os.path.join(ROOT, "dropin", "configs", "reward", "mcia.yaml")).read()
    res = symmetry.conventional_records([])
    assert res[0] == [] and len(res[1]) == 0
