"""CPU checks of the fingerprint-matching layer (matinvent_amd.novelty, include/matinvent_hip_match.h): the header's symbols and
the ctypes table; the group builder and the host validation that stands in front of every upload; leader resolution from a pair matrix;
the bank's padding, alignment and save / load; read_extxyz; UNFilter's refusals and call shape with the kernel call replaced by the numpy
restatement tests/fp_match_ref.py; and the kernels' own source run on the host (scripts/fp_match_host_check.cpp) against that restatement,
the guard included."""
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from matinvent_amd import _lib, novelty
from matinvent_amd import structure as S
from tests import fp_match_ref as R
from tests import fp_ref64
from tests.header_util import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_and_table():
    names = declared_symbols("matinvent_hip_match.h")
    assert names == ["mi_fp_match", "mi_fp_match_plan", "mi_fp_match_workspace"] and sorted(_lib.MATCH_SIGNATURES) == names
    assert any(t is _lib.MATCH_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    import re
    src = open(os.path.join(ROOT, "include", "matinvent_hip_match.h")).read()
    struct = re.search(r"typedef struct mi_fp_match_args \{(.*?)\} mi_fp_match_args;", src, re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    fields = [n for decl in struct.split(";") for n in re.findall(r"\b(\w+)\s*(?:,|$)", decl.strip())]
    assert fields == [f for f, _ in _lib.FpMatchArgs._fields_]
    macro = lambda k: int(re.search(rf"#define {k}\s+([0-9]+)", src).group(1))
    assert (macro("MI_FP_MATCH_TILE"), macro("MI_FP_MATCH_ITEM_INTS")) == (_lib.FP_MATCH_TILE, _lib.FP_MATCH_ITEM_INTS) == (R.TILE, 5)
    assert [R.chain(n) for n in (1, 192, 256, 257, 2304)] == [10, 10, 10, 14, 42]   # L(ncols) as the header states it


def _rec(species, fp=None, flag=0):
    n = len(species)
    return SimpleNamespace(species=list(species), frac_coords=np.zeros((n, 3)), lengths=[4.0, 4.0, 4.0], angles=[90.0, 90.0, 90.0], fp=fp, flag=flag)


def _fake_fingerprints(records, fingerprints, fp_args):
    """memory._fingerprints_of for records that carry their own row: no device."""
    if fingerprints is not None:
        return np.asarray(fingerprints[0], np.float32), np.asarray(fingerprints[1]).astype(np.int64)
    width = 36 * int((fp_args or {}).get("nbins", 64))
    fp = np.zeros((len(records), width), np.float32)
    for i, r in enumerate(records):
        if r.fp is not None and not r.flag:
            fp[i, :len(r.fp)] = r.fp
    return fp, np.array([r.flag for r in records], np.int64)


def _numpy_kernel(calls):
    def run(query, groups, bank, tol, pairs=False, chunk=0):
        calls.append(groups)
        glist = [(list(groups["q_idx"][groups["grp_q_off"][g]:groups["grp_q_off"][g + 1]]),
                  list(groups["c_idx"][groups["grp_c_off"][g]:groups["grp_c_off"][g + 1]]), int(n)) for g, n in enumerate(groups["grp_ncols"])]
        bd, bi, nw, st, mats = R.match_groups(np.asarray(query), glist, bank.host_rows(), bank.host_len, tol)
        return bd.astype(np.float32), bi, nw, st, ([m.astype(np.float32) for m in mats] if pairs else None)
    return run


NB = 5   # nbins of the CPU tests: row lengths 5 -> 8, 15 -> 16, 30 -> 32


def _unit(ncols, seed):
    return R.unit_rows(1, ncols, ncols, seed)[0]


def test_bank_padding_alignment_save_and_load(tmp_path):
    bank = novelty.FingerprintBank(nbins=NB, r_max=3.0, sigma=0.2, device="cpu")
    recs = [_rec([3], _unit(5, 1)), _rec([3, 8, 8], _unit(15, 2)), _rec([3, 8, 26], _unit(30, 3)), _rec([8], _unit(5, 4)),
            _rec([3, 8], flag=2), _rec([11, 17], _unit(15, 5))]
    rows = bank.add(recs, _fake_fingerprints(recs, None, bank.fp_args))
    assert rows == [0, 1, 2, 3, -1, 4] and len(bank) == 5
    assert bank.host_len.tolist() == [8, 16, 32, 8, 16] and bank.host_start.tolist() == [0, 8, 24, 56, 64] and bank.n_floats == 80
    assert (bank.host_start % 4 == 0).all() and bank.start[:5].tolist() == bank.host_start.tolist() and bank.length[:5].tolist() == bank.host_len.tolist()
    for r, rec in zip(bank.host_rows(), [recs[i] for i in (0, 1, 2, 3, 5)]):
        assert (r[:len(rec.fp)] == rec.fp).all() and not r[len(rec.fp):].any()           # zero padding
    assert bank.formulas == ["Cl" + "Na", "FeLiO", "Li", "LiO", "LiO2", "O"] and bank.index["LiO2"] == [1] and bank.flagged == {"LiO": 1}
    more = [_rec([3], _unit(5, 10 + k)) for k in range(200)]                              # the buffers grow by doubling
    bank.add(more, _fake_fingerprints(more, None, bank.fp_args))
    assert len(bank) == 205 and bank.rows.numel() == 2048 and bank.start.numel() == 256 and bank.n_floats == 80 + 1600
    assert (bank.host_rows()[1][:15] == recs[1].fp).all() and bank.index["Li"][:2] == [0, 5]
    path = bank.save(str(tmp_path / "bank.npz"))
    back = novelty.FingerprintBank.load(path, nbins=NB, r_max=3.0, sigma=0.2, device="cpu")
    assert len(back) == len(bank) and back.formulas == bank.formulas and back.flagged == bank.flagged and back.index == bank.index
    assert back.host_len.tolist() == bank.host_len.tolist() and back.host_start.tolist() == bank.host_start.tolist()
    assert (back.rows[:back.n_floats].numpy() == bank.rows[:bank.n_floats].numpy()).all()
    for kw in (dict(nbins=6, r_max=3.0, sigma=0.2), dict(nbins=NB, r_max=8.0, sigma=0.2), dict(nbins=NB, r_max=3.0, sigma=0.15)):
        with pytest.raises(ValueError, match="parameters"):
            novelty.FingerprintBank.load(path, device="cpu", **kw)


def _bank_and_list():
    bank = novelty.FingerprintBank(nbins=NB, device="cpu")
    banked = [_rec([3], _unit(5, 1)), _rec([3, 8], _unit(15, 2)), _rec([3], _unit(5, 3)), _rec([3, 8], flag=4), _rec([3, 8], _unit(15, 6))]
    bank.add(banked, _fake_fingerprints(banked, None, bank.fp_args))
    # formulas interleaved, one absent from the bank (Fe), flagged records (one of a banked formula, one of an absent one)
    recs = [_rec([3, 8], _unit(15, 2)), _rec([3], _unit(5, 7)), _rec([26], _unit(5, 8)), _rec([3, 8], _unit(15, 9)), _rec([3], _unit(5, 3)),
            _rec([3, 8], flag=1), _rec([29, 8], flag=1), _rec([8, 3], _unit(15, 6))]
    return bank, recs


def test_group_builder_and_host_validation():
    bank, recs = _bank_and_list()
    fp, status = _fake_fingerprints(recs, None, bank.fp_args)
    formulas, ncols = [novelty._formula(r) for r in recs], [novelty.record_ncols(r, NB) for r in recs]
    assert ncols == [15, 5, 5, 15, 5, 15, 15, 15]
    g = novelty.build_groups(formulas, ncols, status, bank)
    assert g["formulas"] == ["LiO", "Li", "Fe"] and g["grp_ncols"].tolist() == [15, 5, 5]
    assert g["grp_q_off"].tolist() == [0, 3, 5, 6] and g["q_idx"].tolist() == [0, 3, 7, 1, 4, 2]
    assert g["grp_c_off"].tolist() == [0, 2, 4, 4] and g["c_idx"].tolist() == [1, 3, 0, 2]
    assert all(a.dtype == np.int32 for k, a in g.items() if k != "formulas")
    assert 0 <= g["q_idx"].min() and g["q_idx"].max() < len(recs) and 0 <= g["c_idx"].min() and g["c_idx"].max() < len(bank)
    for k, n in enumerate(g["grp_ncols"]):
        assert (bank.host_len[g["c_idx"][g["grp_c_off"][k]:g["grp_c_off"][k + 1]]] == R.round4(n)).all()
    assert novelty.validate_groups(g, len(recs), fp.shape[1], bank.host_len, ncols)
    empty = novelty.build_groups([], [], [], bank)
    assert empty["grp_q_off"].tolist() == [0] and len(empty["q_idx"]) == 0 and novelty.validate_groups(empty, 0, 4, bank.host_len)

    def corrupt(**kw):
        bad = {k: np.array(v) for k, v in g.items() if k != "formulas"}
        for k, (i, v) in kw.items():
            bad[k][i] = v
        return bad

    for bad, what in ((corrupt(c_idx=(0, 9)), "candidate index"), (corrupt(c_idx=(1, -1)), "candidate index"), (corrupt(q_idx=(2, 8)), "query index"),
                      (corrupt(q_idx=(2, 0)), "more than one"), (corrupt(c_idx=(0, 0)), "length 8"), (corrupt(grp_ncols=(1, 15)), "length"),
                      (corrupt(grp_c_off=(1, 5)), "ascending"), (corrupt(grp_q_off=(3, 7)), "ascending")):
        with pytest.raises(ValueError, match=what):
            novelty.validate_groups(bad, len(recs), fp.shape[1], bank.host_len)
    with pytest.raises(ValueError, match="multiple of 4"):
        novelty.validate_groups(g, len(recs), 182, bank.host_len)


def test_a_corrupted_list_never_reaches_the_library(monkeypatch):
    """The host validation raises before the kernel call: the call is replaced by one that fails the test."""
    bank, recs = _bank_and_list()
    monkeypatch.setattr(novelty, "_fingerprints_of", _fake_fingerprints)
    monkeypatch.setattr(novelty, "_run_kernel", lambda *a, **k: pytest.fail("the library was called with an invalid list"))
    bank.index["LiO"] = [1, 0]                                   # a row of another formula (length 8, not 16)
    with pytest.raises(ValueError, match="length 8"):
        novelty.novel_mask(recs, bank)
    bank.index["LiO"] = [1, 40]                                  # a row that does not exist
    with pytest.raises(ValueError, match="candidate index"):
        novelty.match(recs, bank)


@pytest.mark.parametrize("n", [1, 2, 7, 40])
def test_leader_resolution_is_the_sequential_loop(n):
    g = np.random.default_rng(n)
    for trial in range(20):
        same = g.random((n, n)) < (0.05 + 0.04 * trial)
        same = same | same.T | np.eye(n, dtype=bool)
        d = np.where(same, 0.01, 0.5).astype(np.float32)
        assert novelty.resolve_leaders(d, 0.02) == R.leaders_naive(same)


def test_leader_chain_keeps_both_ends():
    same = np.array([[1, 1, 0], [1, 1, 1], [0, 1, 1]], bool)     # a ~ b, b ~ c, a !~ c
    assert novelty.resolve_leaders(np.where(same, 0.0, 1.0), 0.02) == R.leaders_naive(same) == [0, 2]


def test_read_extxyz_inverts_write_extxyz(tmp_path):
    recs = []
    for name, (t, x, L) in fp_ref64.kernel_cases().items():
        L = np.asarray(L, np.float64)
        ln = np.linalg.norm(L, axis=1)
        ang = [float(np.degrees(np.arccos(np.dot(L[(k + 1) % 3], L[(k + 2) % 3]) / (ln[(k + 1) % 3] * ln[(k + 2) % 3])))) for k in range(3)]
        recs.append(SimpleNamespace(species=[int(z) for z in t], frac_coords=np.asarray(x, np.float64), lengths=ln.tolist(), angles=ang))
    path = S.write_extxyz(recs, str(tmp_path / "cases.extxyz"), infos=[{"reward": k} for k in range(len(recs))])
    back = S.read_extxyz(path)
    assert len(back) == len(recs)
    for k, (a, b) in enumerate(zip(recs, back)):
        assert a.species == b.species and b.info["reward"] == str(k)
        d = a.frac_coords - b.frac_coords
        assert np.abs(d - np.round(d)).max() < 1e-6
        assert np.abs(np.array(a.lengths) - b.lengths).max() < 1e-6 and np.abs(np.array(a.angles) - b.angles).max() < 1e-6
    assert S.reduced_formula(back[3].species) == S.reduced_formula(recs[3].species)


def test_unfilter_refusals():
    for m, needs in (("stable", "MatterSim"), ("synthesizable", "weights")):
        with pytest.raises(ValueError, match=needs):
            novelty.UNFilter(metrics=["unique", m])
    with pytest.raises(ValueError, match="none of"):
        novelty.UNFilter(metrics=["unique", "pretty"])
    f = novelty.UNFilter(metrics=["validity", "novel"], fp_args={"nbins": NB}, some_reference_key=1)
    assert f.metrics == ("novel",) and f._bank is None           # nothing is loaded or launched until it is called


def test_unfilter_call_shape_and_memory(monkeypatch, tmp_path):
    calls = []
    monkeypatch.setattr(novelty, "_fingerprints_of", _fake_fingerprints)
    monkeypatch.setattr(novelty, "_run_kernel", _numpy_kernel(calls))
    bank, recs = _bank_and_list()
    path = bank.save(str(tmp_path / "ref.npz"))
    near = _unit(15, 9).astype(np.float64) + 0.01 * R.unit_rows(1, 15, 15, 99)[0]          # within fp_tol of record 3
    recs.append(_rec([3, 8], (near / np.linalg.norm(near)).astype(np.float32)))
    fp, status = _fake_fingerprints(recs, None, {"nbins": NB})
    formulas = [novelty._formula(r) for r in recs]
    assert R.distance(fp[3], fp[8]) < 0.02 / 2
    want_u = R.unique_mask(formulas, fp, status, 0.02)
    bfp, bst = np.zeros((5, 180), np.float32), np.array([0, 0, 0, 4, 0])
    for k, r in enumerate(bank.host_rows()):
        bfp[[0, 1, 2, 4][k], :len(r)] = r
    want_n = R.novel_mask(formulas, fp, status, ["Li", "LiO", "Li", "LiO", "LiO"], bfp, bst, 0.02)
    assert want_u.tolist() == [True, True, True, True, True, True, True, True, False]
    assert want_n.tolist() == [False, True, True, True, False, False, True, False, True]
    flt = novelty.UNFilter(reference_path=path, remember=True, fp_args={"nbins": NB}, device="cpu")
    data = [f"data{k}" for k in range(len(recs))]
    kept_data, kept, metrics = flt(data, recs, None)
    keep = want_u & want_n
    assert kept == [r for r, k in zip(recs, keep) if k] and kept_data == [d for d, k in zip(data, keep) if k]
    assert set(metrics) == {"unique_frac", "novel_frac", "un_frac", "bank_size"} and all(isinstance(v, float) for v in metrics.values())
    assert metrics["unique_frac"] == want_u.mean() and metrics["novel_frac"] == want_n.mean() and metrics["un_frac"] == keep.mean()
    assert metrics["bank_size"] == 4 + 3 == len(flt.bank) and flt.bank.flagged == {"LiO": 1, "CuO": 1}
    assert len(calls) == 2                                       # one call per mask
    again_data, again, m2 = flt(data, recs, None)                # everything that passed is remembered: nothing is novel twice
    assert again == [] and again_data == [] and m2["novel_frac"] == 0.0 and m2["un_frac"] == 0.0 and m2["bank_size"] == 7.0
    only_u = novelty.UNFilter(metrics=["unique"], fp_args={"nbins": NB}, device="cpu")
    assert only_u(data, recs)[1] == [r for r, k in zip(recs, want_u) if k] and len(only_u.bank) == 0
    assert novelty.UNFilter(fp_args={"nbins": NB}, device="cpu")([], [], None) == ([], [], {"unique_frac": 0.0, "novel_frac": 0.0, "un_frac": 0.0, "bank_size": 0.0})


def test_dropin_path_config_and_package_override():
    import sys
    from matinvent_amd import config as C
    dropin = os.path.join(ROOT, "dropin")
    cfg = C.resolved(C.compose(os.path.join(dropin, "configs"), "base", ["+filter@sample_cfg.filter=un", "sample_cfg.filter.remember=false"]))
    assert cfg.sample_cfg.filter._target_ == "pipeline.filters.un_filter.UNFilter" and cfg.pipeline.sample_cfg.filter.remember is False
    assert "filter" not in C.compose(os.path.join(dropin, "configs"), "base", []).sample_cfg      # nothing is configured by default
    sys.path.insert(0, dropin)
    try:
        flt = C.instantiate(cfg.sample_cfg.filter)
        from pipeline.filters import OptFilter
        from pipeline.filters.un_filter import UNFilter
    finally:
        sys.path.remove(dropin)
    assert isinstance(flt, UNFilter) and UNFilter is novelty.UNFilter and flt.metrics == ("unique", "novel") and not flt.remember
    assert OptFilter()(1, 2) == (1, 2, {})                       # the pass-through stays what it was


# ---- the kernels' own source on the host ------------------------------------------------------------------------------------------------------
def _compiler():
    for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if path:
            return path
    return None


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = _compiler()
    assert cxx is not None, "no host C++ compiler (the ROCm toolchain that builds the library ships one)"
    exe = str(tmp_path_factory.mktemp("fpm") / "fp_match_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "scripts", "fp_match_host_check.cpp"), "-o", exe], check=True)
    return exe


def write_case(path, query, packed, tol, pairs=True, chunk=0):
    Q, stride = query.shape
    with open(path, "wb") as f:
        np.array([Q, stride, len(packed["bank_len"]), len(packed["grp_ncols"]), len(packed["q_idx"]), len(packed["c_idx"]), int(pairs), chunk], np.int32).tofile(f)
        np.array([len(packed["bank"])], np.int64).tofile(f)
        np.array([tol], np.float32).tofile(f)
        for k, dt in (("bank", np.float32), ("bank_start", np.int64), ("bank_len", np.int32), ("grp_q_off", np.int32), ("q_idx", np.int32),
                      ("grp_c_off", np.int32), ("c_idx", np.int32), ("grp_ncols", np.int32)):
            if k == "bank":
                np.ascontiguousarray(query, np.float32).tofile(f)
            np.ascontiguousarray(packed[k], dt).tofile(f)


def read_out(path, Q, packed, pairs=True):
    raw = np.fromfile(path, np.int32)
    nq, nc = np.diff(packed["grp_q_off"]), np.diff(packed["grp_c_off"])
    mats, at = [], 4 * Q
    for a, b in zip(nq, nc):
        mats.append(raw[at:at + a * b].view(np.float32).reshape(a, b) if pairs else None)
        at += a * b if pairs else 0
    assert at == len(raw)
    return raw[:Q].view(np.float32), raw[Q:2 * Q], raw[2 * Q:3 * Q], raw[3 * Q:4 * Q], mats


def run_host(exe, tmp, query, groups, bank_rows, tol, pairs=True, chunk=0, packed=None):
    packed = packed or R.pack(groups, bank_rows)
    write_case(str(tmp / "case.bin"), query, packed, tol, pairs, chunk)
    subprocess.run([exe, str(tmp / "case.bin"), str(tmp / "out.bin")], check=True, stdout=subprocess.DEVNULL)
    return read_out(str(tmp / "out.bin"), len(query), packed, pairs)


def test_host_run_of_the_kernel_source_meets_the_documented_budget(host_check, tmp_path):
    case = R.distance_case()
    bd, bi, nw, st, mats = run_host(host_check, tmp_path, case["query"], case["groups"], case["bank_rows"], R.TOL)
    R.check_distances(case, bd, bi, nw, st, mats, R.TOL, "host")
    again = run_host(host_check, tmp_path, case["query"], case["groups"], case["bank_rows"], R.TOL, chunk=16)   # another cut into chunks: same bits
    assert all(a.tobytes() == b.tobytes() for a, b in zip(mats, again[4])) and bd.tobytes() == again[0].tobytes() and (bi == again[1]).all()
    none = run_host(host_check, tmp_path, case["query"], case["groups"], case["bank_rows"], R.TOL, pairs=False)
    assert bd.tobytes() == none[0].tobytes() and (bi == none[1]).all() and (nw == none[2]).all()


def test_host_run_guard_skips_bad_candidates_without_reading(host_check, tmp_path):
    """Out-of-range and wrong-length candidates, a start that is not a multiple of 4, a row that ends past the bank, a query index out of
    range: skipped, status 1, and (under the sanitizers, scripts/fp_match_host_check.cpp) never read.  This case belongs on the CPU."""
    rows = [R.unit_rows(1, 16, 16, k)[0] for k in range(6)] + [R.unit_rows(1, 8, 8, 9)[0]]
    query = np.zeros((4, 16), np.float32)
    query[0], query[1], query[2, :8] = R.unit_rows(1, 16, 16, 20)[0], rows[2], R.unit_rows(1, 8, 8, 21)[0]
    groups = [([0, 1], [5, 99, 2, -3, 6, 0, 2 ** 31 - 1], 16), ([2], [6, 1], 8), ([3], [], 16)]
    want = R.match_groups(query, groups, rows, [len(r) for r in rows], 0.02)
    bd, bi, nw, st, mats = run_host(host_check, tmp_path, query, groups, rows, 0.02)
    assert st.tolist() == [1, 1, 1, 0] == want[3].tolist() and bi.tolist() == want[1].tolist() == [bi[0], 2, 6, -1] and nw.tolist() == want[2].tolist()
    for m, w in zip(mats, want[4]):
        assert (np.isnan(m) == np.isnan(w)).all() and np.nanmax(np.abs(m - w), initial=0) < 1e-6
    packed = R.pack(groups, rows)
    packed["bank_start"] = packed["bank_start"].copy()
    packed["bank_start"][5] += 2                                 # misaligned
    packed["bank_start"][0] = len(packed["bank"]) - 8            # ends past the bank
    packed["q_idx"] = packed["q_idx"].copy()
    packed["q_idx"][1] = 7                                       # no such query row
    bd2, bi2, nw2, st2, mats2 = run_host(host_check, tmp_path, query, groups, rows, 0.02, packed=packed)
    assert np.isnan(mats2[0][0, [0, 1, 3, 4, 5, 6]]).all() and not np.isnan(mats2[0][0, 2]) and bi2[0] == 2 and st2[0] == 1
    assert (bd2[1], bi2[1], nw2[1], st2[1]) == (np.inf, -1, 0, 0)     # the row of the dropped query position is untouched
