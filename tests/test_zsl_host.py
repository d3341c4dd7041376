"""CPU checks of the substrate matcher that need no GPU (matinvent_amd.substrates, include/matinvent_hip_zsl.h, matinvent_amd/csrc/zsl_match.h;
DESIGN 52): the header, its table and the build list; the numpy restatement tests/zsl_ref64.py against closed forms on a cubic substrate,
against its invariances and against an independent brute force on every case; the margin of every decision; the reward calculator's
argument checks and the drop-in config; and the kernels' text run on the host under the host sanitizers and held to the restatement
(integers and areas bit for bit).  The case lists of tests/test_gpu_zsl.py live in tests/zsl_cases.py."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from matinvent_amd import _lib
from tests import zsl_cases as Z
from tests import zsl_ref64 as R
from tests.header_util import ROOT, declared_symbols

MARGIN = 1e-9   # the smallest |quantity - tolerance| of every case: a last-bit difference in acos flips no decision
INT_KEYS = ("f_mult", "f_status", "s_mult", "s_status", "res_i", "res_n", "mcia_plane", "mcia_status")
BIT_KEYS = ("f_vec", "f_area", "s_vec", "s_area", "mcia")


def compare(ref, got, dev, what, factor=4.0):
    """Every output against the restatement: integers, plane vectors and areas bit for bit; theta and the strains to `factor` x the
    restatement's own deviation from a higher-precision evaluation (zsl_ref64.deviation).  Returns the largest (theta, strain) difference
    as a multiple of that deviation."""
    same = lambda a, b: np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    for k in INT_KEYS + BIT_KEYS:
        if k in got:
            assert same(ref[k], got[k]), (what, k, ref[k], got[k])
    rd, gd = ref["res_d"], np.asarray(got["res_d"])
    for col in (0, 5, 9):   # the two areas (and the padding)
        assert same(rd[..., col], gd[..., col]), (what, "res_d", col)
    strain_cols = [1, 2, 3, 4, 6, 7, 8]
    assert same(np.isnan(rd[..., strain_cols]), np.isnan(gd[..., strain_cols])) and same(np.isinf(rd[..., 4]), np.isinf(gd[..., 4])), what
    fin = np.isfinite(rd[..., strain_cols])
    worst_s = float(np.abs(rd[..., strain_cols][fin] - gd[..., strain_cols][fin]).max()) if fin.any() else 0.0
    worst_t = 0.0
    if "s_table" in got:
        for sp, m in enumerate(ref["s_mult"]):
            n = R.OFFSET[m + 1] if ref["s_status"][sp] != R.BAD_CELL else 0
            a, b = ref["s_table"][sp, :n], np.asarray(got["s_table"])[sp, :n]
            assert same(a[:, :2], b[:, :2]), (what, "s_table lengths", sp)
            worst_t = max(worst_t, float(np.abs(a[:, 2] - b[:, 2]).max()) if n else 0.0)
    assert worst_t <= factor * dev["theta"] and worst_s <= factor * dev["strain"], (what, worst_t, dev["theta"], worst_s, dev["strain"])
    return worst_t / dev["theta"] if dev["theta"] else 0.0, worst_s / dev["strain"] if dev["strain"] else 0.0


def test_header_table_and_build_list():
    from matinvent_amd.build import SOURCES
    names = sorted(declared_symbols("matinvent_hip_zsl.h"))
    assert names == ["mi_zsl_planes", "mi_zsl_reduce", "mi_zsl_search", "mi_zsl_tables", "mi_zsl_workspace"]
    assert sorted(_lib.ZSL_SIGNATURES) == names and any(t is _lib.ZSL_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    assert "zsl.hip" in SOURCES and len(SOURCES) == 31 and len(set(SOURCES)) == 31
    head = open(os.path.join(ROOT, "include", "matinvent_hip_zsl.h")).read()
    ops = open(os.path.join(ROOT, "matinvent_amd", "csrc", "zsl_match.h")).read()
    unit = open(os.path.join(ROOT, "matinvent_amd", "csrc", "zsl.hip")).read()
    assert "fp contract(off)" in ops and "__host__ __device__" in ops and '#include "zsl_match.h"' in unit
    for word in ("atomic", "mfma"):   # no atomics, no matrix pipe
        assert word not in ops and word not in unit.split("namespace mi {", 1)[1], word
    for k, v in (("MAX_MULT", R.MAX_MULT), ("MAX_MILLER", R.MAX_MILLER), ("TABLE", R.TABLE), ("ROW_D", R.ROW_D), ("ROW_I", R.ROW_I)):
        assert f"#define MI_ZSL_{k} {v}" in head and f"ZSL_{k} = {v}" in ops and getattr(_lib, "ZSL_" + k) == v, k
    for code, k in enumerate(("OK", "NO_MATCH", "MULT_CAP", "REDUCE_CAP", "BAD_CELL")):
        assert f"#define MI_ZSL_{k} {code}" in head and f"ZSL_{k} = {code}" in ops and getattr(_lib, "ZSL_" + k) == getattr(R, k) == code
    assert f"ZSL_REDUCE_ITERS = {R.REDUCE_ITERS}" in ops and R.TABLE == sum(R.SIGMA[1:R.MAX_MULT + 1]) and max(R.SIGMA[:R.MAX_MULT + 1]) < 256
    assert os.path.exists(os.path.join(ROOT, "scripts", "zsl_host_check.cpp"))
    # the argument blocks are the header's structs, field for field
    for cls, struct in ((_lib.ZslPlanesArgs, "mi_zsl_planes_args"), (_lib.ZslSearchArgs, "mi_zsl_search_args"), (_lib.ZslReduceArgs, "mi_zsl_reduce_args")):
        body = head[head.index(f"typedef struct {struct}"):head.index(f"}} {struct};")]
        at = -1
        for k, _ in cls._fields_:
            hits = [i for i in (body.find(f" {k};", at + 1), body.find(f"*{k};", at + 1), body.find(f" {k},", at + 1), body.find(f", {k};", at + 1)) if i >= 0]
            assert hits and min(hits) > at, (struct, k)
            at = min(hits)
    # the entries bind, and their host-only refusals answer without a GPU, by name
    lib = _lib.load()
    assert lib.mi_zsl_workspace(3) == 3 * R.TABLE * 24 and lib.mi_zsl_workspace(0) == 0
    assert lib.mi_zsl_workspace(-1) == _lib.MI_EINVAL and b"-1 planes" in lib.mi_last_error()
    for fn in (lib.mi_zsl_planes, lib.mi_zsl_search, lib.mi_zsl_reduce):
        assert fn(None, None) == _lib.MI_EINVAL and b"null argument block" in lib.mi_last_error()
    a = _lib.ZslPlanesArgs()
    a.C, a.P, a.max_area = 1, 13, 0.0
    assert lib.mi_zsl_planes(C.byref(a), None) == _lib.MI_EINVAL and b"max_area" in lib.mi_last_error()
    a.max_area = 400.0
    assert lib.mi_zsl_planes(C.byref(a), None) == _lib.MI_EINVAL and b"null pointer" in lib.mi_last_error()
    a.C = 0
    assert lib.mi_zsl_planes(C.byref(a), None) == 0   # no planes: nothing is launched
    s = _lib.ZslSearchArgs()
    s.B, s.Pf, s.Ps, s.max_area_ratio_tol, s.max_length_tol, s.max_angle_tol = 1, 13, 1, 0.09, -0.03, 0.01
    assert lib.mi_zsl_search(C.byref(s), None) == _lib.MI_EINVAL and b"tolerance" in lib.mi_last_error()
    s.max_length_tol, s.B, s.Pf, s.Ps = 0.03, 1 << 20, 49, 117
    assert lib.mi_zsl_search(C.byref(s), None) == _lib.MI_ECAPACITY and b"items" in lib.mi_last_error()
    s.B = 1
    assert lib.mi_zsl_search(C.byref(s), None) == _lib.MI_EINVAL and b"null pointer" in lib.mi_last_error()
    r = _lib.ZslReduceArgs()
    r.B, r.Pf, r.Ps, r.S = 1, 0, 1, 1
    assert lib.mi_zsl_reduce(C.byref(r), None) == _lib.MI_EINVAL and b"no film plane" in lib.mi_last_error()
    assert lib.mi_zsl_tables(None, None, None, 2, None, None) == _lib.MI_EINVAL and b"null pointer" in lib.mi_last_error()
    assert lib.mi_zsl_tables(None, None, None, 0, None, None) == 0


def test_planes_bases_and_normal_forms():
    from matinvent_amd.substrates import miller_planes
    assert len(R.planes(1)) == 13 and len(R.planes(2)) == 49 and R.planes(1)[:4] == [(0, 0, 1), (0, 1, -1), (0, 1, 0), (0, 1, 1)] and R.planes(1)[-1] == (1, 1, 1)
    for m in (1, 2, 3):
        ps = R.planes(m)
        assert ps == sorted(ps) == miller_planes(m) and len(set(ps)) == len(ps)
        for hkl in ps:
            u, v = basis = R.basis(hkl)
            assert tuple(np.cross(u, v)) == hkl, (hkl, basis)
    for h in range(-8, 9):
        for k in range(-8, 9):
            if h or k:
                g, p, q = R.egcd(h, k)
                assert g == math.gcd(abs(h), abs(k)) and p * h + q * k == g
    for n in range(1, R.MAX_MULT + 1):
        hs = R.hnfs(n)
        assert len(hs) == R.SIGMA[n] and all(i * m == n and 0 <= j < m for i, j, m in hs) and hs == sorted(hs)
    # the reduction: a reduced pair has a.b >= 0, |a| <= |b| <= |b +- a|, and the same area as the pair it came from
    rng = np.random.default_rng(3)
    a, b = rng.normal(size=(200, 3)) * 5.0, rng.normal(size=(200, 3)) * 5.0
    ra, rb, ended = R.reduce_pairs(a, b)
    n2 = lambda x: (x * x).sum(1)
    assert ended.all() and ((ra * rb).sum(1) >= 0).all() and (n2(ra) <= n2(rb)).all() and (n2(rb) <= n2(rb + ra)).all() and (n2(rb) <= n2(rb - ra)).all()
    assert np.allclose(np.linalg.norm(np.cross(ra, rb), axis=1), np.linalg.norm(np.cross(a, b), axis=1), rtol=1e-10)
    long_a, long_b, ended = R.reduce_pairs([[1.0, 0.0, 0.0]], [[1000.5, 1.0, 0.0]])   # a chain of a thousand subtractions: past the cap
    assert not ended[0]


def test_closed_forms_on_a_cubic_substrate():
    ref = Z.reference("closed")
    a2 = float(np.float32(Z.SI_A)) ** 2
    area, status, ri = ref["mcia"][:, 0], ref["mcia_status"][:, 0], ref["res_i"][:, 0]
    assert abs(area[0] - a2) <= 1e-12 * a2 and ri[0, 2] == 1 and ri[0, 3] == 1          # edge a: a^2 at n_f = 1
    assert abs(area[1] - a2) <= 1e-6 * a2 and ri[1, 2] == 2                              # a / sqrt 2 (in float32): a^2 at n_f = 2
    assert abs(area[2] - a2) <= 1e-6 * a2 and ri[2, 2] == 4                              # a / 2: a^2 at n_f = 4
    assert area[3] == 117.0 and ri[3, 2] == 13 and ri[3, 3] == 4                         # edge 3.0: 13 x 9 on 4 x a^2
    assert math.isinf(area[4]) and status[4] == R.NO_MATCH and ri[4, 1] == -1           # every plane area exceeds max_area
    assert status[:4].tolist() == [R.OK] * 4 and np.isnan(ref["res_d"][4, 0, 1:4]).all()
    assert np.abs(ref["res_d"][0, 0, 1:4]).max() == 0.0 and np.abs(ref["res_d"][3, 0, 1:4]).max() <= 0.03
    exact = R.analyze(Z.CLOSED[:1], [(0, 0, 1)], [Z.SI_100])   # the exact match alone: its margin is the angle tolerance
    assert exact["mcia"][0, 0] == area[0] and abs(exact["margin"] - 0.01) < 1e-12, exact["margin"]
    # the inclusive end of the multiples: a plane of area max_area / 2 exactly has n = 1, 2
    assert R.plane(Z.cubic(10.0), (0, 0, 1), 200.0)["mult"] == 2 and R.plane(Z.cubic(10.0), (0, 0, 1), 199.99)["mult"] == 1
    tiny = R.plane(Z.cubic(1.0), (0, 0, 1), 400.0)
    assert tiny["status"] == R.MULT_CAP and tiny["mult"] == R.MAX_MULT


def test_every_case_keeps_its_margin_and_its_guards():
    worst = min(Z.reference(name)["margin"] for name in Z.CASES)
    if os.environ.get("MI_TOL_REPORT"):
        print(f"TOL zsl margin: the smallest |quantity - tolerance| over every case is {worst:.3g}")
    for name in Z.CASES:
        assert Z.reference(name)["margin"] >= MARGIN, (name, Z.reference(name)["margin"])
    g = Z.reference("guards")
    assert g["mcia_status"][:, 0].tolist() == [R.OK, R.BAD_CELL, R.BAD_CELL, R.MULT_CAP, R.OK] and np.isinf(g["mcia"][1:3, 0]).all()
    assert g["mcia"][3, 0] == 29.0 and g["f_status"].reshape(5, 13)[3].tolist() == [R.MULT_CAP] * 13 and (g["f_mult"].reshape(5, 13)[3] == R.MAX_MULT).all()
    assert np.array_equal(g["mcia"][[0, 4], 0], [Z.reference("ortho")["mcia"][0, 0], Z.reference("triclinic")["mcia"][1, 0]])
    t = Z.reference("ties")   # film planes (001), (010), (100) tie on every substrate plane: the lowest key stays
    assert t["res_i"][0, :, 1].tolist() == [0, 0, 0] and len(set(t["res_d"][0, :, 0].tolist())) == 1
    c = Z.reference("ties_count")
    assert c["res_n"][0, 0] == c["res_n"][0, 1] == c["res_n"][0, 2] > 0 and c["res_i"][0, :, 10].tolist() == [0, 0, 0] and not c["res_d"][0, :, 4].any()


@pytest.mark.parametrize("name", sorted(Z.CASES))
def test_the_brute_force_agrees(name):
    """The independent routine (plain loops, recursive reduction, no early exit, one list of every match) on every (film, substrate
    plane) of the case: the same area bit for bit, the same key; in count mode the same count and the same least strained match."""
    films, m, bank, count = Z.CASES[name]
    ref = Z.reference(name)
    hkls = R.planes(m)
    sp = 0
    for lat, shk in bank:
        for hkl in shk:
            for b in range(len(films)):
                if ref["res_i"][b, sp, 0] not in (R.OK, R.NO_MATCH):
                    continue   # (a guard: the brute force has no caps)
                bf = R.brute(films[b], hkls, lat, hkl)
                assert bf["area"] == ref["res_d"][b, sp, 0] and bf["key"] == R.row_key(ref["res_i"][b, sp]), (name, b, sp, bf, ref["res_i"][b, sp])
                if count:
                    assert bf["n_matches"] == ref["res_n"][b, sp] and bf["ls_key"] == R.row_key(ref["res_i"][b, sp], 1), (name, b, sp, bf)
                    assert bf["ls_strain"] == ref["res_d"][b, sp, 4] or (bf["ls_key"] is None and math.isinf(ref["res_d"][b, sp, 4]))
            sp += 1


def test_invariances():
    hk = R.planes(1)
    # A unimodular recombination of the film's rows: Miller indices go over as h' = U h.  The case is built so that the answer cannot
    # leave the plane set: the film matches at n_f = 1 in its plane of smallest area (no plane of any index has a smaller one, and a match
    # area is at least its plane's area), and that plane's image stays inside film_max_miller = 1.
    for film, U in ((Z.ORTHO[2], [[1, 0, 0], [1, 1, 0], [0, 1, 1]]), (Z.cubic(Z.SI_A), [[1, 1, 0], [0, 1, 0], [1, 0, 1]])):
        U = np.array(U)
        assert round(np.linalg.det(U)) == 1
        base = R.analyze([film], hk, [Z.SI_100])
        plane = np.array(hk[int(base["res_i"][0, 0, 1])])
        smallest = min(R.plane(film, h, 400.0)["area"] for h in R.planes(3))
        assert base["res_i"][0, 0, 2] == 1 and base["mcia"][0, 0] == smallest and np.abs(U @ plane).max() == 1
        moved = R.analyze([(U @ film.reshape(3, 3).astype(np.float64)).astype(np.float32).reshape(9)], hk, [Z.SI_100])
        assert abs(moved["mcia"][0, 0] - base["mcia"][0, 0]) <= 1e-12 * base["mcia"][0, 0] and moved["res_i"][0, 0, 2] == 1 and moved["mcia_status"][0, 0] == R.OK
        assert tuple(U @ plane) == hk[int(moved["res_i"][0, 0, 1])]
    # the axes of a cubic substrate swap roles: nothing changes
    for film in (Z.ORTHO[1], Z.TRICLINIC[3]):
        per_plane = [R.analyze([film], hk, [(Z.cubic(Z.SI_A), [p])]) for p in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]
        assert len({float(r["mcia"][0, 0]) for r in per_plane}) == 1 and len({tuple(r["res_i"][0, 0, 1:10]) for r in per_plane}) == 1
    # count mode leaves the lowest match alone
    a, b = Z.reference("ortho"), Z.reference("ortho_count")
    assert np.array_equal(a["res_i"][..., :10], b["res_i"][..., :10]) and np.array_equal(a["res_d"][..., :4], b["res_d"][..., :4], equal_nan=True)
    assert (b["res_n"] >= 1).all() and (b["res_d"][..., 4] <= np.abs(b["res_d"][..., 1:4]).max(-1)).all()


def test_the_reward_calculators_arguments(monkeypatch, tmp_path):
    from matinvent_amd import rewards, substrates
    from matinvent_amd.data import SimpleStructure
    with pytest.raises(ValueError, match="no table of named substrates"):
        rewards.PyMatGen(task="mcia")
    with pytest.raises(ValueError, match="no table of named substrates"):
        rewards.PyMatGen(task="mcia", substrate="Si")
    with pytest.raises(AssertionError):
        rewards.PyMatGen(task="price")
    with pytest.raises(ValueError):
        rewards.PyMatGen(task="mcia", substrate=[5.4437] * 3 + [90.0] * 3, zsl=dict(film_max_miller=4))
    with pytest.raises(ValueError):
        rewards.PyMatGen(task="mcia", substrate=np.eye(3) * 5.0, substrate_millers=[(0, 0, 0)])
    with pytest.raises(ValueError):
        rewards.PyMatGen(task="mcia", substrate=substrates.Substrate("Si", np.eye(3) * 5.4437, [(1, 0, 0)]), substrate_millers=[(1, 0, 0)])
    for bad in (dict(max_area=0.0), dict(max_length_tol=-1.0), dict(max_angle_tol=math.nan), dict(substrate_max_miller=0)):
        with pytest.raises(ValueError):
            substrates.ZSL(**bad)
    z = substrates.ZSL()
    assert (z.max_area, z.max_area_ratio_tol, z.max_length_tol, z.max_angle_tol, z.film_max_miller, z.substrate_max_miller) == (400.0, 0.09, 0.03, 0.01, 1, 1)
    # the four spellings of a cell
    si = SimpleStructure([5.4437] * 3, [90.0] * 3, [14] * 8, np.zeros((8, 3)))
    from matinvent_amd.structure import write_extxyz
    path = write_extxyz([si], str(tmp_path / "si.xyz"))
    cells = [substrates.cell_matrix(c) for c in ([5.4437] * 3 + [90.0] * 3, np.eye(3) * 5.4437, si, path)]
    assert all(c.dtype == np.float32 and c.shape == (3, 3) for c in cells) and all(np.abs(c - cells[1]).max() < 1e-5 for c in cells)
    calc = rewards.PyMatGen(task="mcia", substrate=path, substrate_millers=[[1, 0, 0]], zsl=dict(film_max_miller=2))
    assert calc.substrate.millers == [(1, 0, 0)] and calc.zsl.film_max_miller == 2 and calc.bank is None and not calc.primitive
    assert rewards.PyMatGen(task="mcia", substrate=np.eye(3) * 5.4437).substrate.planes(1) == R.planes(1)
    assert substrates.record_cells([si, "not a crystal"])[0].tolist() == cells[2].reshape(9).tolist() and np.isnan(substrates.record_cells([si, "not a crystal"])[1]).all()
    # NaN on any status other than OK; density keeps its value
    seen = []

    def fake(records, bank, zsl, primitive=False, device="cuda"):
        seen.append((len(records), bank, zsl, primitive))
        return np.array([29.5, math.inf, 117.0, 50.0, 60.0]), np.array([0, 1, 0, 2, 4])

    monkeypatch.setattr(substrates, "mcia", fake)
    calc.bank = "built"
    out = calc.calc(([si] * 5, None))
    assert np.array_equal(out, [29.5, np.nan, 117.0, np.nan, np.nan], equal_nan=True) and seen == [(5, "built", calc.zsl, False)]
    rw = rewards.Reward(str(tmp_path / "rewards"), [dict(name="mcia", calculator=calc, target="descending", minv=0, maxv=180)], 0.8)
    r, props, failed = rw.scoring([si] * 5)
    assert failed.tolist() == [False, True, False, True, True] and abs(r[0] - (1 - 29.5 / 180)) < 1e-12 and r[1] == 0.0
    d = rewards.PyMatGen(task="density").calc([si])
    assert abs(d[0] - 8 * 28.085 * 1.66053906660 / 5.4437 ** 3) < 1e-3


def test_dropin_config():
    text = open(os.path.join(ROOT, "dropin", "configs", "reward", "mcia.yaml")).read()
    assert "_target_: rewards.calculators.PyMatGen" in text and "_target_: rewards.reward.Reward" in text and "task: mcia" in text
    assert "substrate: [5.4437, 5.4437, 5.4437, 90.0, 90.0, 90.0]" in text and "substrate_millers: [[1, 0, 0]]" in text
    assert "target: descending" in text and "minv: 0" in text and "maxv: 180" in text and "reward_threshold: 0.8" in text
    import sys
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        from rewards.calculators import PyMatGen
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
    try:
        import yaml
    except ImportError:
        yaml = None
    if yaml is not None:
        cfg = yaml.safe_load(text)["prop_cfg"][0]["calculator"]
        calc = PyMatGen(**{k: v for k, v in cfg.items() if k != "_target_"})
        assert calc.task == "mcia" and calc.substrate.millers == [(1, 0, 0)] and abs(float(calc.substrate.cell[0, 0]) - 5.4437) < 1e-6


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("zsl") / "zsl_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "zsl_host_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("name", sorted(Z.CASES))
def test_host_check_under_the_host_sanitizers(host_check, tmp_path, name):
    """scripts/zsl_host_check.cpp: zsl_match.h in the kernels' order, built with AddressSanitizer and UndefinedBehaviorSanitizer as a
    stand-alone program -- integers, plane vectors and areas equal to the restatement bit for bit, theta and the strains to 4 x the
    restatement's own deviation, on the fixtures of tests/test_gpu_zsl.py (the guards among them)."""
    films, m, bank, count = Z.CASES[name]
    cf, of = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    R.write_case(cf, films, R.planes(m), bank, None, count)
    r = subprocess.run([host_check, cf, of], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    Ps, S = Z.widths(bank)
    got = R.read_out(of, len(films), len(R.planes(m)), Ps, S)
    ratios = compare(Z.reference(name), got, Z.deviation(name), name)
    if os.environ.get("MI_TOL_REPORT"):
        print(f"TOL zsl host check {name}: theta {ratios[0]:.2f} x, strains {ratios[1]:.2f} x the restatement's deviation")
    ref = Z.reference(name)
    assert f"{len(films)} films x {S} substrates" in r.stdout and f"{int((ref['mcia_status'] != R.OK).sum())} not OK" in r.stdout
