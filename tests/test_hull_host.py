"""CPU checks of the energy above the convex hull that need no GPU (matinvent_amd.stability, include/matinvent_hip_hull.h,
matinvent_amd/csrc/hull_simplex.h): the header, its table and the build list; the numpy restatement tests/hull_ref64.py
against an independent brute-force value and, where scipy is installed, against HiGHS; the kernels' text run on the host under the host
sanitizers and held to the restatement bit for bit; the case lists of tests/test_gpu_hull.py with their tie marks; PhaseBank, SUNFilter
and the reward calculator with the kernel call replaced by the restatement; the drop-in config."""
import ctypes
import os
import shutil
import subprocess
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

from matinvent_amd import _lib, config as C, novelty, stability as S
from tests import hull_ref64 as H
from tests.header_util import ROOT, declared_symbols

EXAMPLE = os.path.join(ROOT, "dropin", "configs")

# |e_hull(restatement) - e_hull(another solver)|, eV/atom on energies of magnitude <= 3.  Measured on the cases of this file: 9.1e-15
# against `brute` (288 queries, d = 1 .. 8, <= 14 candidates) and 1.0e-14 against scipy's HiGHS (160 queries, d = 1 .. 8, 2 d .. 2000
# candidates); the algorithm's prototype measured 1.3e-14 against HiGHS on 896 cases.  The bound is 8 x the largest of the three, rounded.
VALUE_BOUND = 1e-13

# The cases of tests/test_gpu_hull.py: name -> make_case arguments.  Element counts 1, 2, 8; candidate counts d (terminals only),
# 255 / 256 / 257 (the workgroup's stride) and 455 / 456 at d = 8 (9 x 455 = 4095 <= LDS_DOUBLES = 4096 < 9 x 456: the two sides of the
# LDS budget); a query on a bank row's composition (the degenerate vertex); NaN energies scattered through the list.
CASES = {
    "d1": dict(d=1, nc=5, seed=11, nq=3),
    "d2_terminals": dict(d=2, nc=2, seed=12, nq=3),
    "d8_terminals": dict(d=8, nc=8, seed=13, nq=3),
    "d2_255": dict(d=2, nc=255, seed=14, nq=3),
    "d2_256": dict(d=2, nc=256, seed=15, nq=3),
    "d2_257": dict(d=2, nc=257, seed=16, nq=3),
    "d5_700": dict(d=5, nc=700, seed=17, nq=3),
    "d8_455": dict(d=8, nc=455, seed=18, nq=3),
    "d8_456": dict(d=8, nc=456, seed=19, nq=3),
    "d3_on_bank": dict(d=3, nc=40, seed=20, nq=4, on_bank=True),
    "d8_on_bank": dict(d=8, nc=300, seed=21, nq=3, on_bank=True, max_count=2),
    "d4_nan": dict(d=4, nc=300, seed=22, nq=3, nan_frac=0.25),
    "d3_q300": dict(d=3, nc=60, seed=23, nq=300),
}
MANY_GROUPS = 200   # 200 groups of one query: group g has d = 1 + g % 5 elements and d + (7 g) % 23 candidates


@lru_cache(maxsize=None)
def case(name):
    return H.make_case(**CASES[name])


@lru_cache(maxsize=None)
def reference(name):
    """(outputs of run_call over the case's one group, per-query simplex results with their decision gaps)"""
    c, gaps = case(name), []
    out = H.run_call(c["bank"], H.one_group(c), c["query_c"], c["query_e"], gaps)
    return out, [r for _, r in sorted(gaps, key=lambda t: t[0])]


@lru_cache(maxsize=None)
def many_groups():
    cases = [H.make_case(d=1 + g % 5, nc=1 + g % 5 + (7 * g) % 23, seed=1000 + g, nq=1, on_bank=g % 3 == 0) for g in range(MANY_GROUPS)]
    bank, groups, qc, qe = H.merge_cases(cases)
    gaps = []
    out = H.run_call(bank, groups, qc, qe, gaps)
    return bank, groups, qc, qe, out, [r for _, r in sorted(gaps, key=lambda t: t[0])]


def test_header_table_and_build_list():
    from matinvent_amd.build import SOURCES
    names = sorted(declared_symbols("matinvent_hip_hull.h"))
    assert names == ["mi_hull_above", "mi_hull_workspace"]
    assert sorted(_lib.HULL_SIGNATURES) == names and any(t is _lib.HULL_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    assert "hull.hip" in SOURCES
    head = open(os.path.join(ROOT, "include", "matinvent_hip_hull.h")).read()
    text = open(os.path.join(ROOT, "matinvent_amd", "csrc", "hull_simplex.h")).read()
    for k, name in enumerate(("OK", "NO_TERMINAL", "UNBOUNDED", "ITER_CAP", "BAD_QUERY")):
        assert f"#define MI_HULL_{name} {k}" in head and f"HULL_{name} = {k}" in text
    assert (_lib.HULL_OK, _lib.HULL_NO_TERMINAL, _lib.HULL_UNBOUNDED, _lib.HULL_ITER_CAP, _lib.HULL_BAD_QUERY) == (H.OK, H.NO_TERMINAL, H.UNBOUNDED, H.ITER_CAP, H.BAD_QUERY)
    assert (S.OK, S.NO_TERMINAL, S.UNBOUNDED, S.ITER_CAP, S.BAD_QUERY) == (0, 1, 2, 3, 4)
    assert "#define MI_HULL_MAX_ELEMS 8" in head and "#define MI_HULL_MAX_ITERS 256" in head and "#define MI_HULL_EPS 1e-12" in head
    assert "#define MI_HULL_LDS_DOUBLES 4096" in head and "#define HULL_EPS 1e-12" in text and "#define HULL_LDS_DOUBLES 4096" in text
    assert (_lib.HULL_MAX_ELEMS, _lib.HULL_MAX_ITERS, _lib.HULL_EPS, _lib.HULL_LDS_DOUBLES) == (H.MAX_ELEMS, H.MAX_ITERS, H.EPS, H.LDS_DOUBLES) == (8, 256, 1e-12, 4096)
    assert "fp contract(off)" in text
    for f in ("hull_host_check.cpp", "hull_timing.py", "build_phase_bank.py"):
        assert os.path.exists(os.path.join(ROOT, "scripts", f))
    # the argument block is the header's struct, field for field
    fields = [k for k, _ in _lib.HullArgs._fields_]
    body = head[head.index("typedef struct mi_hull_args"):head.index("} mi_hull_args")]
    at = -1
    for k in fields:
        nxt = min(i for i in (body.find(f" {k};", at + 1), body.find(f"*{k};", at + 1), body.find(f" {k},", at + 1)) if i >= 0)
        assert nxt > at, k
        at = nxt
    # the entries bind, and their host-only refusals answer without a GPU
    lib = _lib.load()
    assert lib.mi_hull_workspace(-1, 0, 0) == _lib.MI_EINVAL and lib.mi_hull_workspace(0, 0, 0) > 0
    assert lib.mi_hull_workspace(3, 10, 100) >= 100 * 9 * 8 + 100 * 4 + 10 * 4 + 3 * 4
    assert lib.mi_hull_above(None, None) == _lib.MI_EINVAL and b"null argument block" in lib.mi_last_error()
    a = _lib.HullArgs()
    a.max_elems = 1
    assert lib.mi_hull_above(ctypes.byref(a), None) == _lib.MI_EINVAL and b"null" in lib.mi_last_error()
    for k, _ in _lib.HullArgs._fields_[:21]:
        setattr(a, k, 64)   # (a non-null, aligned address that is never used: every refusal below comes before any launch)
    a.Q = -1
    assert lib.mi_hull_above(ctypes.byref(a), None) == _lib.MI_EINVAL and b"negative count" in lib.mi_last_error()
    a.Q = 0
    for bad in (0, 9):
        a.max_elems = bad
        assert lib.mi_hull_above(ctypes.byref(a), None) == _lib.MI_EINVAL and b"max_elems" in lib.mi_last_error()
    a.max_elems = 8
    a.workspace = 68
    assert lib.mi_hull_above(ctypes.byref(a), None) == _lib.MI_EINVAL and b"aligned" in lib.mi_last_error()
    a.workspace = 64
    assert lib.mi_hull_above(ctypes.byref(a), None) == 0   # Q == 0: MI_OK without a launch


def test_the_restatement_agrees_with_brute_force():
    """Every d-subset of <= 14 candidates solved and filtered for l >= 0: no simplex in the comparison value."""
    worst, n = 0.0, 0
    for d in range(1, 9):
        for seed in range(12):
            nc = min(14, max(d, d + seed % (15 - d)))
            c = H.make_case(d, nc, seed * 31 + d, nq=3, on_bank=seed % 2 == 1)
            X, E, _, skipped = H.stage(c["bank"], c["gZ"], c["cand"])
            assert not skipped
            for q in range(3):
                r = H.simplex(X, E, c["query_c"][q][:d], c["query_e"][q])
                assert r["status"] == H.OK and r["iters"] <= 30
                worst, n = max(worst, abs(r["e_hull"] - H.brute(X, E, c["query_c"][q][:d]))), n + 1
                cert = H.certificate(X, E, c["query_c"][q][:d], r["decomp_pos"], r["decomp_frac"], r["e_hull"])
                assert cert["primal"] <= 1e-13 and cert["lam_min"] >= 0 and cert["dual"] >= -1e-11 and cert["value"] <= 1e-13
    print(f"restatement against brute: {n} queries, largest |difference| {worst:.3g} (bound {VALUE_BOUND:g})")
    assert n == 288 and worst <= VALUE_BOUND


def test_the_restatement_agrees_with_highs():
    linprog = pytest.importorskip("scipy.optimize").linprog
    worst, n = 0.0, 0
    for d in range(1, 9):
        for nc, seed in ((2 * d, 1), (64, 2), (257, 3), (456, 4), (2000, 5)):
            for on_bank in (False, True):
                c = H.make_case(d, nc, 100 * d + seed, nq=2, on_bank=on_bank, nan_frac=0.1 if seed == 3 else 0.0)
                X, E, _, _ = H.stage(c["bank"], c["gZ"], c["cand"])
                fin = np.isfinite(E)
                for q in range(2):
                    r = H.simplex(X, E, c["query_c"][q][:d])
                    lp = linprog(E[fin], A_eq=X[fin].T, b_eq=c["query_c"][q][:d], bounds=(0, None), method="highs")
                    assert lp.status == 0 and r["status"] == H.OK
                    worst, n = max(worst, abs(lp.fun - r["e_hull"])), n + 1
    print(f"restatement against HiGHS: {n} queries, largest |difference| {worst:.3g} (bound {VALUE_BOUND:g})")
    assert worst <= VALUE_BOUND


def test_special_statuses_of_the_restatement():
    c = H.make_case(3, 30, 5, nq=2)
    X, E, _, _ = H.stage(c["bank"], c["gZ"], c["cand"])
    pure1 = np.flatnonzero(X[:, 1] == 1.0)
    r = H.simplex(np.delete(X, pure1, axis=0), np.delete(E, pure1), c["query_c"][0][:3])
    assert r["status"] == H.NO_TERMINAL and np.isnan(r["e_hull"]) and np.isnan(r["chempot"]).all() and (r["decomp_pos"] == -1).all()
    E2 = E.copy()
    E2[pure1] = np.nan
    assert H.simplex(X, E2, c["query_c"][0][:3])["status"] == H.NO_TERMINAL
    assert H.simplex(X, E, [0.5, np.nan, 0.5])["status"] == H.BAD_QUERY and H.simplex(X, E, [1.5, -0.5, 0.0])["status"] == H.BAD_QUERY
    r = H.simplex(X, E, c["query_c"][0][:3], np.nan)
    assert r["status"] == H.OK and np.isfinite(r["e_hull"]) and np.isnan(r["e_above"])
    # d = 1: no pivot, the lowest pure energy
    c1 = case("d1")
    X1, E1, _, _ = H.stage(c1["bank"], c1["gZ"], c1["cand"])
    r = H.simplex(X1, E1, [1.0], 0.25)
    assert r["iters"] == 0 and r["e_hull"] == E1.min() and r["e_above"] == 0.25 - E1.min()
    # a row that cannot leave (a direction without a positive component) is UNBOUNDED, not a loop: guards against bad rows
    r = H.simplex(np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, -1.0]]), np.array([0.0, 0.0, -1.0]), [0.5, 0.5])
    assert r["status"] == H.UNBOUNDED


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_committed_cases_end_ok_and_carry_their_tie_marks(name):
    """What tests/test_gpu_hull.py demands of its inputs, checked here first: on the restatement alone every query ends OK, its certificate
    holds, and the cases that must be untied (or tied) are."""
    c = case(name)
    out, res = reference(name)
    d = c["d"]
    assert (out["status"] == H.OK).all() and (out["flags"] == 0).all() and out["iters"].max() <= 40
    X, E, rows, _ = H.stage(c["bank"], c["gZ"], c["cand"])
    for q, r in enumerate(res):
        cert = H.certificate(X, E, c["query_c"][q][:d], r["decomp_pos"], r["decomp_frac"], r["e_hull"])
        assert cert["primal"] <= 1e-13 and cert["lam_min"] >= 0 and cert["dual"] >= -1e-11 and cert["value"] <= 1e-13, (name, q, cert)
    marks = [H.untied(r) for r in res]
    if name in ("d1", "d2_terminals", "d8_terminals"):
        assert all(marks), (name, marks)
    if not CASES[name].get("on_bank"):
        assert any(marks), (name, marks)           # bit equality with the device is asserted on the untied queries
    if name == "d3_on_bank":
        assert not all(marks)                      # the degenerate vertex: the leaving row is tied
    if name == "d3_q300":
        assert sum(marks) >= 150
    if name == "d4_nan":
        assert np.isnan(c["bank"]["energy"]).sum() >= 40
    if name in ("d8_455", "d8_456"):
        assert (9 * 455 <= H.LDS_DOUBLES < 9 * 456) and out["iters"].min() >= 4


def test_many_groups_reference():
    bank, groups, qc, qe, out, res = many_groups()
    assert len(groups["grp_nelem"]) == MANY_GROUPS == len(qe) and (out["status"] == H.OK).all()
    assert set(groups["grp_nelem"].tolist()) == {1, 2, 3, 4, 5} and sum(H.untied(r) for r in res) >= 100


# ---- the kernels' text on the host ------------------------------------------------------------------------------------------------------------
def write_case(path, bank, groups, qc, qe, no_lds=0):
    i32, f64 = (lambda x: np.ascontiguousarray(x, np.int32).tobytes()), (lambda x: np.ascontiguousarray(x, np.float64).tobytes())
    with open(path, "wb") as f:
        f.write(i32([len(bank["nelem"]), len(groups["grp_nelem"]), len(qe), len(groups["q_idx"]), len(groups["c_idx"]), no_lds]))
        f.write(i32(bank["nelem"]) + i32(bank["Z"]) + f64(bank["frac"]) + f64(bank["energy"]))
        f.write(i32(groups["grp_nelem"]) + i32(groups["grp_Z"]) + i32(groups["grp_q_off"]) + i32(groups["q_idx"]) + i32(groups["grp_c_off"]) + i32(groups["c_idx"]))
        f.write(f64(qc) + f64(qe))


def read_out(path, Q):
    raw = open(path, "rb").read()
    assert len(raw) == Q * (18 * 8 + 11 * 4)
    f, i = np.frombuffer(raw[:Q * 18 * 8], np.float64), np.frombuffer(raw[Q * 18 * 8:], np.int32).astype(np.int64)
    return dict(e_hull=f[:Q], e_above=f[Q:2 * Q], chempot=f[2 * Q:10 * Q].reshape(Q, 8), decomp_frac=f[10 * Q:].reshape(Q, 8),
                decomp_idx=i[:8 * Q].reshape(Q, 8), iters=i[8 * Q:9 * Q], status=i[9 * Q:10 * Q], flags=i[10 * Q:])


def assert_same_outputs(got, want, where=""):
    for k in S.OUTPUT_KEYS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k]), equal_nan=np.asarray(want[k]).dtype.kind == "f"), (where, k)


def corrupted_call():
    """One call with everything the guard must survive: a candidate index past the bank and a negative one, a row with a foreign element,
    a row with n_elem = 9 and one with a fraction that is not finite, a group with d = 0, one with d = 9, one whose element list descends,
    one whose offsets leave the lists, a query index outside 0 .. Q - 1, a query of NaN energy and one with a NaN fraction."""
    cases = [H.make_case(d=2 + g, nc=20 + 5 * g, seed=300 + g, nq=2) for g in range(7)]
    bank, groups, qc, qe = H.merge_cases(cases)
    bank = {k: v.copy() for k, v in bank.items()}
    M = len(bank["nelem"])
    c_off, c_idx = groups["grp_c_off"], groups["c_idx"].copy()
    c_idx[c_off[0] + 3], c_idx[c_off[0] + 7] = M + 5, -2
    c_idx[c_off[1] + 2] = c_idx[c_off[2] + 1]                                       # a row of group 2's elements in group 1
    bank["nelem"][c_idx[c_off[1] + 9]] = 9
    r = c_idx[c_off[1] + 11]
    bank["frac"][r, 0] = np.inf
    groups = dict(groups, c_idx=c_idx, grp_nelem=groups["grp_nelem"].copy(), grp_Z=groups["grp_Z"].copy(), q_idx=groups["q_idx"].copy())
    groups["grp_nelem"][2] = 0
    groups["grp_nelem"][3] = 9
    groups["grp_Z"][4][:2] = groups["grp_Z"][4][:2][::-1]
    groups["grp_c_off"] = groups["grp_c_off"].copy()
    groups["grp_c_off"][7] = len(c_idx) + 5
    groups["q_idx"][1] = len(qe) + 3
    qe, qc = qe.copy(), qc.copy()
    qe[2] = np.nan
    qc[3, 0] = np.nan
    return bank, groups, qc, qe


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("hull") / "hull_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "hull_host_check.cpp"), "-o", exe], check=True)
    return exe


def _host_run(exe, tmp_path, bank, groups, qc, qe, no_lds=0):
    cf, of = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    write_case(cf, bank, groups, qc, qe, no_lds)
    r = subprocess.run([exe, cf, of], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return read_out(of, len(qe)), r.stdout


def test_host_check_under_the_host_sanitizers(host_check, tmp_path):
    """scripts/hull_host_check.cpp: csrc/hull_simplex.h in the kernels' order, thread by thread, built with AddressSanitizer and
    UndefinedBehaviorSanitizer as a stand-alone program -- equal to the restatement in every output, bit for bit, on every committed case,
    on both staging paths, over many groups and on the corrupted call."""
    for name in sorted(CASES):
        c = case(name)
        for no_lds in (0, 1):
            got, log = _host_run(host_check, tmp_path, c["bank"], H.one_group(c), c["query_c"], c["query_e"], no_lds)
            assert_same_outputs(got, reference(name)[0], (name, no_lds))
            big = (c["d"] + 1) * len(c["cand"]) > H.LDS_DOUBLES
            assert (", 0 blocks in LDS" in log) == bool(no_lds or big), log
    bank, groups, qc, qe, want, _ = many_groups()
    assert_same_outputs(_host_run(host_check, tmp_path, bank, groups, qc, qe)[0], want, "many groups")
    bank, groups, qc, qe = corrupted_call()
    got, log = _host_run(host_check, tmp_path, bank, groups, qc, qe)
    want = H.run_call(bank, groups, qc, qe)
    assert_same_outputs(got, want, "corrupted")
    assert "2 groups with a skipped candidate" in log
    # rows 0 (group 0) flagged and solved; row 1 (bad query index) untouched; row 2 e_q NaN; row 3 BAD_QUERY; groups 2 .. 4 and 6 untouched
    assert want["flags"].tolist() == [1, 0, 1, 1] + [0] * 10 and want["status"].tolist() == [0, -1, 0, H.BAD_QUERY] + [-1] * 6 + [0, 0, -1, -1]
    assert np.isfinite(want["e_hull"][2]) and np.isnan(want["e_above"][2])


def test_skipped_candidates_change_nothing_else():
    """The results of a list with a bad index and a foreign row equal those of the list without them."""
    c = case("d4_nan")
    other = H.make_case(3, 6, 77, elems=[95, 96, 97])
    bank = {k: np.concatenate([c["bank"][k], other["bank"][k]]) for k in c["bank"]}
    M = len(bank["nelem"])
    dirty = np.concatenate([c["cand"][:50], [M + 1], c["cand"][50:200], [len(c["cand"]) + 4], c["cand"][200:], [-1]]).astype(np.int32)
    a = H.run_call(bank, H.one_group(c, dirty), c["query_c"], c["query_e"])
    b = H.run_call(bank, H.one_group(c), c["query_c"], c["query_e"])
    assert (a["flags"] == 1).all() and (b["flags"] == 0).all()
    for k in S.OUTPUT_KEYS:
        if k != "flags":
            assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- PhaseBank, energy_above_hull, SUNFilter (the kernel call replaced by the restatement) -------------------------------------------------------------
def _rec(species):
    return SimpleNamespace(species=list(species))


def _numpy_kernel(calls):
    def run(bank, groups, query_c, query_e, no_lds=False):
        calls.append(groups)
        return H.run_call(bank.arrays(), groups, query_c, query_e)
    return run


def toy_bank(device="cpu"):
    """Li (3) and O (8): Li -1.0 (and a worse polymorph -0.9), O -2.0, Li2O -3.0, LiO -2.9 (both on the hull); a NaN row; an unrelated Fe row."""
    recs = [_rec([3]), _rec([3, 3]), _rec([8, 8]), _rec([3, 3, 8]), _rec([3, 8]), _rec([3, 8, 8, 8]), _rec([26])]
    return S.PhaseBank.from_records(recs, [-1.0, -0.9, -2.0, -3.0, -2.9, np.nan, -4.0], device=device)


def test_phase_bank_round_trip_and_candidate_cache(tmp_path):
    bank = toy_bank()
    assert len(bank) == 7 and bank.nelem.tolist() == [1, 1, 1, 2, 2, 2, 1] and bank.Z[3].tolist() == [3, 8, 0, 0, 0, 0, 0, 0]
    assert bank.frac[3, 0] == 2 / 3 and bank.frac[3, 1] == 1 / 3 and bank.frac[0, 0] == 1.0 and np.isnan(bank.energy[5])
    assert bank.candidates([8, 3]).tolist() == [0, 1, 2, 3, 4, 5] and bank.candidates([3]).tolist() == [0, 1] and bank.candidates([26, 8]).tolist() == [2, 6]
    assert bank.candidates([47]).tolist() == [] and bank.candidates((3, 8)) is bank.candidates([3, 8])        # cached per set
    hit = bank.candidates([3, 8])
    assert bank.add([_rec([8, 8, 8]), _rec(range(1, 10))], [-1.5, 0.0]) == [7, -1] and bank.dropped == 1
    assert bank.candidates([3, 8]) is not hit and bank.candidates([3, 8]).tolist() == [0, 1, 2, 3, 4, 5, 7]  # invalidated by add
    total = S.PhaseBank(device="cpu")
    total.add([_rec([3, 3, 8])], [-9.0], per_atom=False)
    assert total.energy.tolist() == [-3.0]
    back = S.PhaseBank.load(bank.save(str(tmp_path / "phases.npz")), device="cpu")
    for k, v in bank.arrays().items():
        assert np.array_equal(v, back.arrays()[k], equal_nan=True) and v.dtype == back.arrays()[k].dtype, k
    with np.load(str(tmp_path / "phases.npz"), allow_pickle=False) as z:
        assert sorted(z.files) == ["Z", "energy", "frac", "nelem"]                                              # data only
    assert np.array_equal(S.element_mask([1, 63, 64, 118]), np.array([(1 << 1) | (1 << 63), (1 << 0) | (1 << 54)], np.uint64))
    with pytest.raises(ValueError, match="energies for"):
        bank.add([_rec([3])], [1.0, 2.0])
    with pytest.raises(ValueError, match="without atoms"):
        bank.add([_rec([])], [1.0])
    with pytest.raises(RuntimeError, match="runs on the GPU"):
        bank.device_arrays()
    np.savez(str(tmp_path / "bad.npz"), nelem=np.array([1]), Z=np.zeros((1, 4)), frac=np.zeros((1, 8)), energy=np.zeros(1))
    with pytest.raises(ValueError, match="inconsistent"):
        S.PhaseBank.load(str(tmp_path / "bad.npz"), device="cpu")


def test_energy_above_hull_by_hand(monkeypatch):
    calls = []
    monkeypatch.setattr(S, "_run_kernel", _numpy_kernel(calls))
    bank = toy_bank()
    recs = [_rec([3, 8, 8]), _rec([3] * 9 + [8]), _rec(range(1, 10)), _rec([3, 3, 8, 3, 3, 8]), _rec([47]), _rec([8]), _rec([3, 8])]
    res = S.energy_above_hull(recs, [-2.0, -1.0, -1.0, -2.95, 0.0, np.nan, -2.9], bank)
    # LiO2 lies between LiO (-2.9) and O (-2.0): 2/3 x -2.9 + 1/3 x -2.0 = -2.6; Li9O between Li and Li2O: 0.7 x -1 + 0.3 x -3 = -1.6
    assert res["e_hull"][0] == pytest.approx(-2.6, abs=1e-14) and res["e_above"][0] == pytest.approx(0.6, abs=1e-14)
    assert res["e_hull"][1] == pytest.approx(-1.6, abs=1e-14) and sorted(res["decomp_idx"][1][:2].tolist()) == [0, 3]
    assert sorted(res["decomp_idx"][0][:2].tolist()) == [2, 4] and res["decomp_idx"][0][2:].tolist() == [-1] * 6
    assert res["e_hull"][3] == -3.0 and res["e_above"][3] == pytest.approx(0.05, abs=1e-14)         # on Li2O's composition
    assert res["status"].tolist() == [S.OK, S.OK, S.NOT_RUN, S.OK, S.NO_TERMINAL, S.NOT_RUN, S.OK]
    assert np.isnan(res["e_above"][[2, 4, 5]]).all() and res["e_above"][6] == 0.0
    assert len(calls) == 1 and len(calls[0]["grp_nelem"]) == 2 and calls[0]["q_idx"].tolist() == [0, 1, 3, 6, 4]   # groups in order of first appearance
    assert res["elements"][0].tolist() == [3, 8, 0, 0, 0, 0, 0, 0]
    total = S.energy_above_hull(recs[:1], [-6.0], bank, per_atom=False)
    assert total["e_above"][0] == res["e_above"][0]
    assert S.stable_mask(res).tolist() == [False, False, False, True, False, False, True]
    assert S.stable_mask(res, threshold=0.02).tolist() == [False, False, False, False, False, False, True]
    assert S.STABLE_THRESHOLD == 0.1 and "UPSTREAM-UNVERIFIED" in open(S.__file__).read()
    with pytest.raises(ValueError, match="energies for"):
        S.energy_above_hull(recs, [0.0], bank)
    empty = S.energy_above_hull([], [], bank)
    assert all(len(empty[k]) == 0 for k in S.OUTPUT_KEYS)


def test_sunfilter_refusals_and_laziness():
    with pytest.raises(ValueError, match="synthesizable"):
        S.SUNFilter(metrics=["stable", "synthesizable"], phase_path="x.npz")
    with pytest.raises(ValueError, match="none of"):
        S.SUNFilter(metrics=["pretty"])
    with pytest.raises(ValueError, match="phase_path"):
        S.SUNFilter()
    with pytest.raises(ValueError, match="threshold"):
        S.SUNFilter(phase_path="x.npz", threshold=float("nan"))
    f = S.SUNFilter(metrics=["validity", "stable", "novel"], phase_path="/nowhere/phases.npz", some_reference_key=1)
    assert f.metrics == ("stable", "novel") and f._bank is None and f.un._bank is None and f.un.metrics == ("novel",)   # nothing loaded or launched
    with pytest.raises(ValueError, match="mlip_opt"):
        f([1, 2], ["a", "b"], None)
    with pytest.raises(ValueError, match="not built"):      # UNFilter keeps refusing "stable"
        novelty.UNFilter(metrics=["stable"])


def test_sunfilter_call_shape_and_metrics(monkeypatch):
    calls = []
    monkeypatch.setattr(S, "_run_kernel", _numpy_kernel(calls))
    n = 6
    uniq, novel = np.array([1, 1, 0, 1, 1, 1], bool), np.array([1, 1, 1, 0, 1, 1], bool)
    monkeypatch.setattr(novelty, "_fingerprints_of", lambda recs, fp, args: (np.zeros((len(recs), 4), np.float32), np.zeros(len(recs), np.int64)))
    monkeypatch.setattr(novelty, "unique_mask", lambda recs, *a, **k: uniq[:len(recs)])
    monkeypatch.setattr(novelty, "novel_mask", lambda recs, *a, **k: novel[:len(recs)])
    monkeypatch.setattr(novelty.UNFilter, "bank", property(lambda self: _FakeFpBank()))
    flt = S.SUNFilter(bank=toy_bank(), threshold=0.1, device="cpu")
    recs = [_rec([3, 3, 8]), _rec([3, 8]), _rec([3, 8]), _rec([3, 8, 8]), _rec([47]), _rec([3, 3, 8])]
    energies = [-2.95, -2.75, -2.9, -2.45, -1.0, -2.5]    # e_above 0.05, 0.15, 0.0, 0.15, NaN (no terminal), 0.5
    data, strucs, m = flt(list("abcdef"), recs, energies)
    assert data == ["a"] and strucs == [recs[0]]          # stable: 0, 2; unique drops 2; the order is the input's
    assert m["stable_frac"] == pytest.approx(2 / n) and m["no_terminal"] == 1.0 and m["sun_frac"] == pytest.approx(1 / n) and m["phase_bank_size"] == 7.0
    assert m["e_above_hull_mean"] == pytest.approx(np.mean([0.05, 0.15, 0.0, 0.15, 0.5]), abs=1e-12)
    assert {"unique_frac", "novel_frac", "un_frac", "bank_size"} <= set(m) and m["un_frac"] == pytest.approx(4 / n)
    assert len(flt.last_result["e_above"]) == n and flt.last_result["status"][4] == S.NO_TERMINAL
    only_s = S.SUNFilter(metrics=["stable"], bank=toy_bank(), threshold=0.2, device="cpu")
    data, strucs, m = only_s(None, recs, energies)
    assert data is None and strucs == [recs[0], recs[1], recs[2], recs[3]] and m["stable_frac"] == pytest.approx(4 / n)
    data, strucs, m = only_s([], [], [])
    assert (data, strucs) == ([], []) and m["stable_frac"] == 0.0 and m["phase_bank_size"] == 7.0
    un_only = S.SUNFilter(metrics=["unique", "novel"], device="cpu")
    data, strucs, m = un_only(list("abcdef"), recs, None)  # no energies needed without "stable"
    assert data == ["a", "b", "e", "f"] and np.isnan(m["stable_frac"]) and len(calls) == 2


class _FakeFpBank:
    fp_args = {}

    def __len__(self):
        return 0

    def add(self, *a):
        return []


def test_e_above_hull_reward(monkeypatch, tmp_path):
    from matinvent_amd import rewards
    monkeypatch.setattr(S, "_run_kernel", _numpy_kernel([]))
    recs = [_rec([3, 3, 8]), _rec([47]), _rec([3, 8])]
    calc = rewards.EAboveHull(bank=toy_bank())
    v = calc.calc((recs, [-2.95, -1.0, -2.7]))
    assert v[0] == pytest.approx(0.05, abs=1e-12) and np.isnan(v[1]) and v[2] == pytest.approx(0.2, abs=1e-12)
    relaxed = rewards.EAboveHull(bank=toy_bank(), relaxer=lambda s, p=None: (s, [-3.0, -1.0, -2.9]))
    assert relaxed.calc(recs)[[0, 2]].tolist() == [0.0, 0.0]
    r = rewards.Reward(root_dir=str(tmp_path / "rewards"), reward_threshold=0.5,
                       prop_cfg=[dict(name="e_above_hull", calculator=calc, target="descending", minv=0.0, maxv=0.5)])
    score, props, failed = r.scoring((recs, [-2.95, -1.0, -2.7]))
    assert score == pytest.approx([0.9, 0.0, 0.6], abs=1e-12) and failed.tolist() == [False, True, False]
    with pytest.raises(ValueError, match="exactly one"):
        rewards.EAboveHull()
    with pytest.raises(ValueError, match="no energies"):
        calc.calc(recs)
    assert len(calc.calc([])) == 0


def test_build_phase_bank_script(tmp_path):
    import importlib.util
    from matinvent_amd.data import SimpleStructure
    from matinvent_amd.structure import write_extxyz
    strucs = [SimpleStructure([4.0, 4.0, 4.0], [90.0, 90.0, 90.0], [3, 3, 8], np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5]], float)),
              SimpleStructure([3.0, 3.0, 3.0], [90.0, 90.0, 90.0], [8], np.zeros((1, 3)))]
    path = write_extxyz(strucs, str(tmp_path / "in.extxyz"), infos=[{"energy": -3.0}, {"energy": -2.0}])
    spec = importlib.util.spec_from_file_location("build_phase_bank", os.path.join(ROOT, "scripts", "build_phase_bank.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    bank = mod.main([path, str(tmp_path / "out.npz"), "--device", "cpu"])
    assert bank.energy.tolist() == [-3.0, -2.0] and bank.nelem.tolist() == [2, 1]
    assert mod.main([path, str(tmp_path / "tot.npz"), "--device", "cpu", "--total"]).energy.tolist() == [-1.0, -2.0]
    assert len(S.PhaseBank.load(str(tmp_path / "out.npz"), device="cpu")) == 2
    with pytest.raises(SystemExit, match="no info field"):
        mod.main([path, str(tmp_path / "x.npz"), "--energy-key", "e_dft"])


def test_dropin_config_composes():
    cfg = C.resolved(C.compose(EXAMPLE, "base", ["+filter@sample_cfg.filter=sun", "sample_cfg.filter.phase_path=/banks/phases.npz", "sample_cfg.filter.threshold=0.05"]))
    m = cfg.sample_cfg.filter
    assert m["_target_"] == "pipeline.filters.sun_filter.SUNFilter" and m.phase_path == "/banks/phases.npz" and m.threshold == 0.05
    assert list(m.metrics) == ["stable", "unique", "novel"] and m.per_atom is True and m.remember is True and m.reference_path is None
    import sys
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        from pipeline.filters.sun_filter import SUNFilter
        assert SUNFilter is S.SUNFilter
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
    doc = open(os.path.join(ROOT, "matinvent_amd", "pipeline.py")).read()
    assert "stability / synthesizability metrics of SUN are out of scope" not in doc and "stability.SUNFilter" in doc
