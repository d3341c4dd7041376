"""CPU checks of composition validity that need no GPU (matinvent_amd.chemistry, include/matinvent_hip_chem.h): the issue's table
of known compositions under the restatement (tests/chem_ref.py, itertools and numpy forms equal), the synthetic edge cases, the kernels'
order run on the host under the sanitizers against the restatement, the loader's refusals, invalid_filter with and without `smact`, the
abundance tasks, and the header with its table and build list."""
import json
import logging
import math
import os
import shutil
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from matinvent_amd import _lib
from matinvent_amd import chemistry as CH
from tests import chem_cases as CS
from tests import chem_ref as R
from tests.header_util import ROOT, declared_symbols

POISON = -77


def both(types, table, **kw):
    """The restatement's row under itertools, asserted equal to the numpy form."""
    a, b = R.one(types, table, method="itertools", **kw), R.one(types, table, method="numpy", **kw)
    assert a == b
    return a


# ---- the rule, on the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CS.NAMED))
def test_known_compositions(name):
    types, kw, expected = CS.NAMED[name]
    row = both(types, CS.TEST_TABLE, **kw)
    for k, v in expected.items():
        got = R.STATUS[row[k]] if k == "status" else row[k]
        assert got == v, (name, k, got, v)
    if name == "Fe3O4":   # one state per element: no mixed valence
        assert row["n_neutral"] == 0
    if name == "SiC":     # of the two neutral combinations, the one with C negative
        assert row["first_ox"][:2] == [-4, 4] and row["elems"][:2] == [6, 14] and row["n_valid"] == 1
    if name == "Li4O2":
        assert row["elems"][:2] == [3, 8] and row["first_ox"][:2] == [1, -2]
    if name == "NaK_no_alloys":
        assert row["first_ox"][:2] == [-1, 1]   # K has no higher electronegativity than Na: the Pauling test holds with Na negative


def test_pauling_tie_missing_and_zero_states():
    tie = {"H": {"ox": [1], "eneg": 2.0}, "He": {"ox": [-1], "eneg": 2.0}}
    row = both([1, 2], tie)
    assert row["n_neutral"] == 1 and row["n_valid"] == 0 and not row["valid"]   # strict: equal ranks fail
    assert both([1, 2], tie, use_pauling_test=False)["valid"]
    missing = {"H": {"ox": [1], "eneg": 1.0}, "He": {"ox": [-1], "eneg": None}}
    assert not both([1, 2], missing)["valid"] and both([1, 2], missing, use_pauling_test=False)["valid"]
    # an unranked element fails the test even where it takes no part in a pair
    spectator = {"H": {"ox": [1], "eneg": 1.0}, "He": {"ox": [-1], "eneg": 3.0}, "Li": {"ox": [0], "eneg": None}}
    assert not both([1, 2, 3], spectator)["valid"]
    # zero states are ignored: Li's rank lies between, on the wrong side of both
    zero = {"H": {"ox": [1], "eneg": 1.0}, "He": {"ox": [-1], "eneg": 3.0}, "Li": {"ox": [0], "eneg": 9.0}, "Be": {"ox": [0], "eneg": 0.1}}
    row = both([1, 2, 3, 4], zero)
    assert row["valid"] and row["first"] == 0 and row["first_ox"][:4] == [1, -1, 0, 0]
    wrong = {"H": {"ox": [1], "eneg": 3.0}, "He": {"ox": [-1], "eneg": 1.0}}
    assert not both([1, 2], wrong)["valid"]


def test_max_combos_edge_and_every_status():
    types, _, _ = CS.NAMED["NH3"]
    N = 16
    assert both(types, CS.TEST_TABLE, max_combos=N)["status"] == R.CODE["ENUMERATED"]
    row = both(types, CS.TEST_TABLE, max_combos=N - 1)
    assert row["status"] == R.CODE["TOO_MANY_COMBOS"] and row["n_combos"] == N and not row["valid"] and row["first"] == -1
    nine = CS.synthetic([2] * 9, [0] * 9)
    seen = {R.STATUS[both(t, tab, **kw)["status"]] for t, tab, kw in (
        ([11, 17], CS.TEST_TABLE, {}), ([14] * 8, CS.TEST_TABLE, {}), ([11, 19], CS.TEST_TABLE, {}), ([0, 8], CS.TEST_TABLE, {}), ([], CS.TEST_TABLE, {}),
        (list(range(1, 10)), nine, {}), ([11, 92], CS.TEST_TABLE, {}), ([2, 8], CS.TEST_TABLE, {}), (types, CS.TEST_TABLE, dict(max_combos=3)))}
    assert seen == set(R.STATUS)
    row = both(list(range(1, 10)) * 2, nine)   # nine elements, two atoms each: the first eight, the counts divided by the gcd of all
    assert row["n_elems"] == 9 and row["elems"] == list(range(1, 9)) and row["counts"] == [1] * 8 and R.STATUS[row["status"]] == "TOO_MANY_ELEMENTS"


def test_atom_ox_follows_a_permutation():
    rng = np.random.default_rng(3)
    types = CS.formula(Fe=4, O=6)
    base = both(types, CS.TEST_TABLE)
    assert base["valid"] and base["counts"][:2] == [3, 2]
    for _ in range(3):
        perm = rng.permutation(len(types))
        row = both([types[i] for i in perm], CS.TEST_TABLE)
        assert row["atom_ox"] == [base["atom_ox"][i] for i in perm]
        assert {k: v for k, v in row.items() if k != "atom_ox"} == {k: v for k, v in base.items() if k != "atom_ox"}


def test_chunk_edge_placements_on_the_restatement():
    for name, table, types, index in CS.chunk_edge_cases():
        row = R.one(types, table, method="numpy")
        assert (row["n_neutral"], row["n_valid"], row["first"]) == (1, 1, index), name
    assert [math.prod(r) for r in CS.CHUNK_RADICES] == [65520, 65536, 65550]


# ---- the kernels' order on the host, under the sanitizers -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("chem") / "chem_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "chem_host_check.cpp"), "-o", exe], check=True)
    return exe


def run_host_check(exe, tmp_path, crystals, table, use_pauling_test=True, include_alloys=True, max_combos=10_000_000, grid=7, node_off=None):
    t = CH.ElementTable(table)
    types = np.array([z for c in crystals for z in c], np.int32)
    off = np.concatenate([[0], np.cumsum([len(c) for c in crystals])]).astype(np.int32) if node_off is None else np.asarray(node_off, np.int32)
    B, N = len(off) - 1, len(types)
    cf, of = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(cf, "wb") as f:
        f.write(struct.pack("<iiiiiq", B, N, int(use_pauling_test), int(include_alloys), grid, max_combos))
        for arr in (t.present, t.n_states, t.ox, t.eneg_rank, t.is_metal, off, types):
            f.write(np.ascontiguousarray(arr, np.int32).tobytes())
    r = subprocess.run([exe, cf, of], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw, pos, out = open(of, "rb").read(), 0, {}
    for k, shape, dt in (("valid", (B,), np.int32), ("status", (B,), np.int32), ("n_elems", (B,), np.int32), ("elems", (B, 8), np.int32), ("counts", (B, 8), np.int32),
                         ("n_combos", (B,), np.int64), ("n_neutral", (B,), np.int64), ("n_valid", (B,), np.int64), ("first", (B,), np.int64),
                         ("first_ox", (B, 8), np.int32), ("atom_ox", (N,), np.int32)):
        size = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[k] = np.frombuffer(raw[pos:pos + size], dt).reshape(shape)
        pos += size
    assert pos == len(raw)
    out["valid"] = out["valid"] == 1
    return out


def assert_rows_equal(got, ref, what=""):
    for k in R.KEYS:
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])


def test_host_check_equals_the_restatement(host_check, tmp_path):
    crystals = [CS.NAMED[n][0] for n in CS.NAMED if not CS.NAMED[n][1]] + CS.shuffled_sizes()
    for kw in ({}, dict(include_alloys=False), dict(use_pauling_test=False), dict(max_combos=15)):
        assert_rows_equal(run_host_check(host_check, tmp_path, crystals, CS.TEST_TABLE, **kw), R.batch(crystals, CS.TEST_TABLE, **kw), kw)
    for table, types in (({"H": {"ox": [1], "eneg": 2.0}, "He": {"ox": [-1], "eneg": 2.0}}, [[1, 2]]),
                         ({"H": {"ox": [1], "eneg": 1.0}, "He": {"ox": [-1], "eneg": None}}, [[1, 2]]),
                         ({"H": {"ox": [1], "eneg": 1.0}, "He": {"ox": [-1], "eneg": 3.0}, "Li": {"ox": [0], "eneg": 9.0}, "Be": {"ox": [0], "eneg": 0.1}}, [[1, 2, 3, 4]]),
                         (CS.synthetic([2] * 9, [0] * 9), [list(range(1, 10)) * 2, list(range(1, 9))])):
        for kw in ({}, dict(use_pauling_test=False)):
            assert_rows_equal(run_host_check(host_check, tmp_path, types, table, **kw), R.batch(types, table, **kw))


def test_host_check_at_the_chunk_edges(host_check, tmp_path):
    for name, table, types, index in CS.chunk_edge_cases():
        got = run_host_check(host_check, tmp_path, [types], table, grid=3)
        assert_rows_equal(got, R.batch([types], table), name)
        assert got["first"][0] == index


def test_host_check_on_the_guard_batch(host_check, tmp_path):
    crystals, names = CS.guard_batch()
    ref = R.batch(crystals, CS.TEST_TABLE)
    assert [R.STATUS[s] for s in ref["status"]] == names
    got = run_host_check(host_check, tmp_path, crystals, CS.TEST_TABLE)
    assert_rows_equal(got, ref)
    # offsets that leave the list: the crystal is BAD_INPUT, nothing is read through them, its atom rows keep the poison; its neighbours stand
    good = [CS.NAMED["NaCl"][0], CS.NAMED["Fe2O3"][0], CS.NAMED["NH3"][0]]
    off = [0, 2, 99, 11]
    got = run_host_check(host_check, tmp_path, good, CS.TEST_TABLE, node_off=off)
    assert [R.STATUS[s] for s in got["status"]] == ["ENUMERATED", "BAD_INPUT", "BAD_INPUT"] and got["first"][0] == 5
    assert (got["atom_ox"][2:] == POISON).all() and got["atom_ox"][:2].tolist() == [1, -1]


# ---- the loader ---------------------------------------------------------------------------------------------------------------------------------------
def test_element_table_ranks_and_refusals(tmp_path):
    t = CH.ElementTable(CS.TEST_TABLE)
    rows, rank = R.by_z(CS.TEST_TABLE)
    for z in range(1, 119):
        assert t.present[z] == (z in rows)
        if z in rows:
            assert t.ox[z, :t.n_states[z]].tolist() == rows[z][0] and t.eneg_rank[z] == rank[z] and t.is_metal[z] == rows[z][2]
    assert t.eneg_rank[R.Z_OF["Si"]] == t.eneg_rank[R.Z_OF["Cu"]] and t.eneg_rank[R.Z_OF["He"]] == -1 and t.eneg_rank[R.Z_OF["K"]] == 0
    assert t.present.dtype == t.ox.dtype == t.eneg_rank.dtype == np.int32 and t.ox.shape == (119, 32)
    p = tmp_path / "table.json"
    p.write_text(json.dumps({"elements": CS.TEST_TABLE}))
    assert np.array_equal(CH.ElementTable.load(str(p)).ox, t.ox)
    for bad, match in (({"Xx": {"ox": [1]}}, "unknown symbol"), ({"Na": {"ox": [1, 1]}}, "duplicate"), ({"Na": {"ox": [128]}}, "out of range"),
                       ({"Na": {"ox": [-128]}}, "out of range"), ({"Na": {"ox": list(range(33))}}, "longer than 32"), ({"Na": {"ox": [1], "eneg": float("inf")}}, "non-finite"),
                       ({"Na": {"ox": [1], "eneg": float("nan")}}, "non-finite"), ({"Na": {"ox": [1.5]}}, "not an integer"), ({"Na": {"oxidation": [1]}}, "unknown key")):
        with pytest.raises(ValueError, match=match):
            CH.ElementTable(bad)
    with pytest.raises(ValueError, match="elements"):
        CH.ElementTable.from_dict({"Na": {"ox": [1]}})
    assert CH.ElementTable({"Na": {"ox": list(range(32))}}).n_states[11] == 32
    with pytest.raises(ValueError, match="max_combos"):
        CH.SmactValidity(t, max_combos=0)
    with pytest.raises(ValueError, match="keys"):
        CH.SmactValidity({"tabel": "x.json"})
    v = CH.SmactValidity({"table": str(p), "include_alloys": False, "max_combos": 1000})
    assert (v.include_alloys, v.use_pauling_test, v.max_combos) == (False, True, 1000) and isinstance(v.table, CH.ElementTable)
    assert CH.make_smact(None) is None and CH.make_smact(v) is v and CH.make_smact(str(p)).max_combos == 10_000_000
    assert v([]).shape == (0,)


def test_build_element_table_script(tmp_path):
    ox, csvf, metals, out = (tmp_path / n for n in ("ox.txt", "eneg.csv", "metals.txt", "table.json"))
    ox.write_text("# symbol then its oxidation states\nNa 1\nCl -1 1 3 5 7\nHe\nFe 2 3  # iron\n")
    csvf.write_text("symbol,eneg,abundance\nNa,0.93,23600\nCl,3.16,145\nHe,,0.008\nFe,1.83,56300\n")
    metals.write_text("Na Fe\n# the rest are not\n")
    r = subprocess.run(["python", os.path.join(ROOT, "scripts", "build_element_table.py"), "--oxidation-states", str(ox), "--properties", str(csvf), "--metals", str(metals),
                        "--out", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    d = json.loads(out.read_text())["elements"]
    assert d["Cl"] == {"ox": [-1, 1, 3, 5, 7], "eneg": 3.16, "metal": False, "abundance": 145.0} and d["He"] == {"ox": [], "eneg": None, "metal": False, "abundance": 0.008}
    assert d["Fe"]["metal"] is True and d["Fe"]["ox"] == [2, 3]
    t = CH.ElementTable.load(str(out))
    assert t.n_states[26] == 2 and t.eneg_rank[2] == -1


# ---- the consumers ------------------------------------------------------------------------------------------------------------------------------------
def _records():
    geo = lambda edge, dist, vol: {"max_cell_edge": edge, "min_distance": dist, "volume": vol}
    return [SimpleNamespace(geometry=geo(5.0, 2.0, 100.0), species=[11, 17]), SimpleNamespace(geometry=geo(30.0, 2.0, 100.0), species=[11, 17]),
            SimpleNamespace(geometry=geo(5.0, 2.0, 100.0), species=[11, 11, 17]), SimpleNamespace(geometry=geo(5.0, 0.1, 100.0), species=[11, 11, 17])]


def test_invalid_filter_with_and_without_smact(caplog):
    from matinvent_amd import filters
    recs = _records()
    calls = []

    def smact(records):   # the restatement stands in for the device: this test is about the wiring
        calls.append(len(records))
        return R.batch([r.species for r in records], CS.TEST_TABLE)["valid"]

    filters._warned.clear()
    with caplog.at_level(logging.WARNING):
        assert filters.invalid_filter(recs, return_mask=True, smact=smact).tolist() == [True, False, False, False]
    assert calls == [4] and "BYPASSED" not in caplog.text and not filters._warned
    data, strucs = filters.invalid_filter(recs, list("abcd"), smact=smact)
    assert data == [recs[0]] and strucs == ["a"]
    with caplog.at_level(logging.WARNING):
        assert filters.invalid_filter(recs, return_mask=True).tolist() == [True, False, True, False]   # the parent's mask
        filters.invalid_filter(recs, return_mask=True)
    assert caplog.text.count("invalid_filter: SMACT charge-neutrality test is BYPASSED (its element database is not available); only the geometric tests "
                             "(cell edge < 25 A, shortest distance > 0.5 A, volume > 0.1 A^3) are applied, so compositions the reference would reject pass") == 1
    assert calls == [4, 4]


def test_filters_and_pipelines_take_smact(tmp_path):
    from matinvent_amd import pipeline
    from matinvent_amd.novelty import UNFilter, validity_first
    from matinvent_amd.stability import SUNFilter
    from matinvent_amd.suite import DiffCSPSuite
    p = tmp_path / "table.json"
    p.write_text(json.dumps({"elements": CS.TEST_TABLE}))
    assert UNFilter(metrics=["validity", "unique"]).validity is False and UNFilter(metrics=["unique"], smact=str(p)).validity is False
    f = SUNFilter(metrics=["validity", "unique"], smact={"table": str(p), "include_alloys": False})
    assert f.validity is True and f.smact.include_alloys is False and UNFilter(metrics=["validity"], smact=str(p)).validity is True
    recs = _records()
    smact = lambda records: R.batch([r.species for r in records], CS.TEST_TABLE)["valid"]
    seen = []

    def inner(data, strucs, energies):
        seen.append((data, strucs, None if energies is None else list(energies)))
        return data, strucs, {"unique_frac": 1.0}

    data, strucs, m = validity_first(smact, inner, list("abcd"), recs, [0.1, 0.2, 0.3, 0.4])
    assert data == ["a", "b"] and strucs == recs[:2] and m == {"unique_frac": 1.0, "valid_frac": 0.5} and seen[0][2] == [0.1, 0.2]
    assert validity_first(smact, inner, [], [], None)[2]["valid_frac"] == 0.0
    suite = DiffCSPSuite("diffcsp", {"batch_size": 4, "num_batches": 1}, {}, device="cpu")
    rl = pipeline.ReinL(rl_epoch=1, model_suite=suite, reward=None, sample_cfg={"smact": {"table": str(p), "max_combos": 500}}, finetune_cfg={}, save_dir=str(tmp_path),
                        save_freq=1, device="cpu")
    assert isinstance(rl.smact, CH.SmactValidity) and rl.smact.max_combos == 500 and np.isnan(rl._smact_log()["smact_valid_frac"])
    plain = pipeline.ReinL(rl_epoch=1, model_suite=suite, reward=None, sample_cfg={}, finetune_cfg={}, save_dir=str(tmp_path), save_freq=1, device="cpu")
    assert plain.smact is None and plain._smact_log() == {}
    text = open(os.path.join(ROOT, "dropin", "configs", "validity", "smact.yaml")).read()
    assert "smact:" in text and "table: null" in text and "max_combos: 10000000" in text


def test_abundance_tasks(tmp_path):
    from matinvent_amd import rewards
    from matinvent_amd.structure import MASSES
    p = tmp_path / "table.json"
    p.write_text(json.dumps({"elements": dict(CS.TEST_TABLE, Mg={"ox": [2], "eneg": 1.31, "metal": True, "abundance": 0.0})}))
    s = lambda species: SimpleNamespace(species=species, lengths=[4.0] * 3, angles=[90.0] * 3)
    strucs = [s([11, 17]), s([26, 26, 8, 8, 8]), s([29, 8]), s([12]), s([92, 8])]
    m_na, m_cl = MASSES[11], MASSES[17]
    want0 = (m_na * 23600.0 + m_cl * 145.0) / (m_na + m_cl)
    want1 = (2 * MASSES[26] * 56300.0 + 3 * MASSES[8] * 461000.0) / (2 * MASSES[26] + 3 * MASSES[8])
    a = rewards.PyMatGen(task="abundance", element_table=str(p)).calc((strucs, None))
    assert np.allclose(a[:2], [want0, want1], rtol=1e-12, atol=0.0)
    assert np.isnan(a[2:]).all()   # Cu: no value; Mg alone: not positive; U: not in the table
    la = rewards.PyMatGen(task="log_abundance", element_table=CH.ElementTable.load(str(p))).calc((strucs, None))
    assert np.allclose(la[:2], np.log10([want0, want1]), rtol=1e-12, atol=0.0) and np.isnan(la[2:]).all()
    with pytest.raises(ValueError, match="element_table"):
        rewards.PyMatGen(task="abundance")
    with pytest.raises(AssertionError):
        rewards.PyMatGen(task="price")


# ---- the header, the table, the unit ------------------------------------------------------------------------------------------------------------------
def test_header_table_constants_and_the_unit():
    from matinvent_amd.build import ALL_SOURCES, MORE_SOURCES, SOURCES
    names = sorted(declared_symbols("matinvent_hip_chem.h"))
    assert names == ["mi_chem_validity", "mi_chem_workspace"] and sorted(_lib.CHEM_SIGNATURES) == names
    assert any(t is _lib.CHEM_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    assert "chem_valid.hip" in MORE_SOURCES and "chem_valid.hip" in ALL_SOURCES and len(SOURCES) == 31 and len(set(ALL_SOURCES)) == len(ALL_SOURCES)
    head = open(os.path.join(ROOT, "include", "matinvent_hip_chem.h")).read()
    enum = open(os.path.join(ROOT, "matinvent_amd", "csrc", "chem_enum.h")).read()
    unit = open(os.path.join(ROOT, "matinvent_amd", "csrc", "chem_valid.hip")).read()
    for name, value in (("MAX_Z", 118), ("MAX_STATES", 32), ("MAX_ELEMS", 8), ("CHUNK", 65536), ("MAX_GRID", 2048), ("MAX_BATCH", 4096), ("DEFAULT_MAX_COMBOS", 10000000)):
        assert f"#define MI_CHEM_{name} {value}" in head and getattr(_lib, "CHEM_" + name) == value
    for code, name in enumerate(CH.STATUS_NAMES):
        assert f"#define MI_CHEM_{name} {code}\n" in head and getattr(_lib, "CHEM_" + name) == code == R.CODE[name] and f"CHEM_{name} = {code}" in enum
    assert (CH.MAX_ELEMS, CH.MAX_STATES, CH.CHUNK) == (R.MAX_ELEMS, R.MAX_STATES, R.CHUNK) and CH.SYMBOLS == R.SYMBOLS
    assert head.count("[UPSTREAM-UNVERIFIED]") >= 1 and '#include "chem_enum.h"' in unit and unit.count("__launch_bounds__(CHEM_THREADS)") == 3
    for word in ("atomic", "mfma", "asm", "float", "double"):   # integers only; plain C++
        assert word not in enum, word
    for word in ("atomic", "mfma", "asm"):
        assert word not in unit.split("namespace mi {", 1)[1], word
    fields = [f[0] for f in _lib.ChemArgs._fields_]
    import re
    body = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    order = [body.index(" " + f + ";") for f in fields if f not in ("B", "N", "use_pauling_test", "include_alloys")]   # the struct's members in the table's order
    assert order == sorted(order) and body.index(" atom_ox;") < body.index(" max_combos;") < body.index("int B, N;") < body.index("int use_pauling_test, include_alloys;")
    # the entries bind and the host-only refusals answer without a GPU
    lib = _lib.load()
    assert lib.mi_chem_validity(None, None) == _lib.MI_EINVAL
    assert lib.mi_chem_workspace(-1, 10) == _lib.MI_EINVAL and lib.mi_chem_workspace(4097, 10) == _lib.MI_EINVAL and lib.mi_chem_workspace(1, 0) == _lib.MI_EINVAL
    assert lib.mi_chem_workspace(1, 2 ** 40 + 1) == _lib.MI_EINVAL and lib.mi_chem_workspace(4096, 2 ** 40) == _lib.MI_EINVAL
    assert lib.mi_chem_workspace(256, 10_000_000) > 256 * 153 * 24 and lib.mi_chem_workspace(0, 1) == 16
    a = _lib.ChemArgs()
    a.B, a.N, a.max_combos = 0, 0, 10
    assert lib.mi_chem_validity(a, None) == _lib.MI_EINVAL   # null pointers are refused before B == 0 is looked at
