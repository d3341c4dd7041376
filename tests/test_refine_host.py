"""CPU-only: the refined structure's definition in its executable form tests/refine_ref64.py -- the orbits of the known crystals
and of a constructed 64-atom Pm-3m cell, exact inputs that do not move, perturbed crystals whose refined copies carry the whole group at a
hundredth of the tolerance, transformed copies, the guards -- the kernel's order run on the host under the sanitizers
(scripts/sym_refine_host_check.cpp), every output equal to the restatement bit for bit, and the host module with the C calls replaced by the
restatement."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import conv_ref64 as CV
from tests import refine_cases as RC
from tests import refine_ref64 as V
from tests import sm_cases as K
from tests import sm_ref64 as R
from tests import sym_cases as C
from tests import sym_ref64 as S
from tests.header_util import ROOT

# The largest relative deviation of a cell parameter between a perturbed crystal and its transformed copy, both refined in the conventional
# cell under the restatement (float32 cells), measured at 1.192e-7 on rocksalt_conv: the bound is four times that.
INVARIANCE_MEASURED = 1.192e-7
INVARIANCE_BOUND = 4 * INVARIANCE_MEASURED
POISON = -7


def rows_of(batch, b):
    return int(batch[0][b]), int(batch[0][b + 1])


def orbit_table(batch, ref, b):
    """[(atoms of the orbit, site order)] in the order of the orbits' lowest atoms."""
    lo, hi = rows_of(batch, b)
    orbit, mult, site = ref["orbit"][lo:hi], ref["mult"][lo:hi], ref["site_order"][lo:hi]
    table = []
    for o in sorted(set(int(v) for v in orbit)):
        members = [i for i in range(hi - lo) if orbit[i] == o]
        assert o == members[0] and all(mult[i] == len(members) for i in members) and len(set(int(site[i]) for i in members)) == 1
        table.append((len(members), int(site[o])))
    return table


def test_orbits_of_the_known_crystals():
    names, batch, ch = RC.regular_results()
    ref = ch["ref"]
    for name, table in RC.KNOWN_ORBITS.items():
        b = names.index(name)
        assert ref["info"][b, 7] == S.OK and orbit_table(batch, ref, b) == table and ref["info"][b, 0] == len(table), name
        lo, hi = rows_of(batch, b)
        z = batch[1][lo:hi]
        assert all(z[i] == z[ref["orbit"][lo + i]] for i in range(hi - lo)), name   # an orbit is of one species
    b = names.index("triclinic")
    lo, hi = rows_of(batch, b)
    assert ref["info"][b].tolist() == [hi - lo, 1, 0, 0, 0, 0, 0, S.OK] and ref["orbit"][lo:hi].tolist() == list(range(hi - lo))
    b = names.index("triclinic_2x1x1")
    assert orbit_table(batch, ref, b) == [(2, 1)] * 3 and ref["info"][b, :2].tolist() == [3, 2]
    b = names.index("one_atom_cubic")
    assert orbit_table(batch, ref, b) == [(1, 48)]


def test_exact_inputs_do_not_move():
    """In float64 from the crystals as they are typed (no float32 rounding of the interface in between)."""
    known = C.known_crystals()
    crystals = [v[0] for v in known.values()] + [RC.pm3m_64()]
    ch = V.chain_exact(crystals, RC.SYMPREC, K.COS_TOL)
    ref = ch["ref"]
    assert (ref["info"][:, 7] == S.OK).all() and ref["info"][:, 1].tolist() == [v[1] for v in known.values()] + [48]
    print("largest move of an exact input: %.3e, largest cell change %.3e" % (ref["stat"][:, 0].max(), ref["stat"][:, 2].max()))
    assert ref["stat"][:, 0].max() <= 1e-12 and ref["stat"][:, 2].max() <= 1e-12


def test_perturbed_crystals_are_refined_onto_the_group():
    names, batch, ch = RC.regular_results()
    ref, F = ch["ref"], ch["F"]
    assert RC.SYMPREC_TIGHT >= 100 * float(np.spacing(np.float32(20.0))) / 2
    clean = {n: V.analyse([RC.base(n)], RC.SYMPREC)[0] for n in RC.PERTURBED}
    for suffix, source in (("~", RC.perturbed()), ("~T", {n: c for n, (c, _) in RC.transformed().items()})):
        idx = [names.index(n + suffix) for n in RC.PERTURBED]
        tight_in = V.analyse([source[n] for n in RC.PERTURBED], RC.SYMPREC_TIGHT)
        tight_out = V.analyse([V.crystal_of(batch, ref, b) for b in idx], RC.SYMPREC_TIGHT)
        for n, b, ti, to in zip(RC.PERTURBED, idx, tight_in, tight_out):
            n_ops, pg, st = clean[n]
            # the conditions: the group of the unperturbed crystal at symprec, fewer operations at the tight tolerance
            assert st == S.OK and F["info"][b][[0, 7]].tolist() == [n_ops, S.OK] and S.PG_NAMES[F["info"][b][4] - 1] == pg, (n, suffix)
            assert ti[0] < n_ops, (n, suffix, ti)
            # the certificate
            assert to == (n_ops, pg, S.OK), (n, suffix, to)
            e = ref["extra"][b]
            Gbar = np.array(e["Gbar"])
            dev = max(np.abs(np.array(V.congruence([int(v) for v in W], e["Gbar"])) - Gbar).max() for W in e["rot"])
            move, cell = V.again(e, len(e["f"]))
            print("%s%s: invariance of Gbar %.2e, second refinement moves %.2e (cell %.2e), max_move %.3e of tol %.3e" %
                  (n, suffix, dev / np.abs(Gbar).max(), move, cell, ref["stat"][b, 0], ch["tol"][b]))
            assert dev <= 1e-12 * np.abs(Gbar).max() and move <= 1e-12 and cell <= 1e-12, (n, suffix)
            assert 0.0 < ref["stat"][b, 1] <= ref["stat"][b, 0] <= 2 * ch["tol"][b] and ref["stat"][b, 3] <= ch["tol"][b], (n, suffix)


def test_transformed_copies():
    names, batch, ch = RC.regular_results()
    ref = ch["ref"]
    for n in RC.PERTURBED:
        a, b = names.index(n + "~"), names.index(n + "~T")
        perm = RC.transformed()[n][1]
        la, lb = rows_of(batch, a), rows_of(batch, b)
        mapped = {frozenset(perm[i] for i in g) for g in V.partition(ref["orbit"][lb[0]:lb[1]])}
        assert mapped == V.partition(ref["orbit"][la[0]:la[1]]), n
        assert sorted(ref["mult"][la[0]:la[1]].tolist()) == sorted(ref["mult"][lb[0]:lb[1]].tolist())
    crystals = [RC.perturbed()[n] for n in RC.PERTURBED] + [RC.transformed()[n][0] for n in RC.PERTURBED]
    out = V.chain_cell(K.batch(crystals), RC.SYMPREC, K.COS_TOL, "conventional")
    k = len(RC.PERTURBED)
    assert (out["info"][:, 7] == S.OK).all()
    dev = {n: float(np.abs(np.array(V.cell_parameters(out["lat"][i + k])) / np.array(V.cell_parameters(out["lat"][i])) - 1.0).max()) for i, n in enumerate(RC.PERTURBED)}
    print({n: "%.3e" % v for n, v in dev.items()})
    assert max(dev.values()) <= INVARIANCE_BOUND < 1e-5, dev


def test_guards():
    """At the entry: a crystal the prepare guard rejected has its info row and nothing else; a crystal whose analysis is not OK is copied."""
    batch, ch = RC.guard_results(POISON)
    ref, P, F = ch["ref"], ch["P"], ch["F"]
    assert [int(P["info"][b][3]) != R.PREP_OK for b in range(6)] == [False, True, True, False, False, False]
    assert ref["info"][0].tolist() == [2, 16, 0, 0, 0, 0, 0, S.OK] and ref["info"][5].tolist() == [2, 192, 0, 0, 0, 0, 0, S.OK]
    for b in (1, 2):
        lo, hi = rows_of(batch, b)
        assert ref["info"][b].tolist() == [0] * 7 + [S.NOT_PREPARED | V.REFINE_FAIL] and (ref["stat"][b] == 0).all()
        assert (ref["frac"][lo:hi] == POISON).all() and (ref["lat"][b] == POISON).all() and (ref["orbit"][lo:hi] == POISON).all()
    assert F["info"][3][7] == S.OPS_CAP and F["info"][4][7] & S.AMBIGUOUS
    for b in (3, 4):
        lo, hi = rows_of(batch, b)
        assert ref["info"][b, 7] == int(F["info"][b][7]) | V.REFINE_FAIL and ref["info"][b, 0] == hi - lo and (ref["stat"][b] == 0).all()
        assert np.array_equal(ref["frac"][lo:hi].view(np.uint32), batch[2][lo:hi].view(np.uint32)) and np.array_equal(ref["lat"][b].view(np.uint32), batch[3][b].view(np.uint32))
        assert ref["orbit"][lo:hi].tolist() == list(range(hi - lo)) and (ref["mult"][lo:hi] == 1).all() and (ref["site_order"][lo:hi] == 1).all()
    assert (ref["trans_ref"][1:5] == POISON).all() and (ref["trans_ref"][0, 16:] == POISON).all() and (ref["trans_ref"][0, :16] != POISON).all()
    # through refine_arrays' rule every guard crystal is unchanged, bit for bit, with the fail bit and one orbit per atom
    out = V.chain_cell(batch, RC.SYMPREC, K.COS_TOL, "given", fill=POISON)
    for b in (1, 2, 3, 4):
        lo, hi = rows_of(batch, b)
        assert out["info"][b, 7] & V.REFINE_FAIL and out["orbit"][lo:hi].tolist() == list(range(hi - lo)) and (out["mult"][lo:hi] == 1).all()
        assert np.array_equal(out["frac"][lo:hi].view(np.uint32), batch[2][lo:hi].view(np.uint32)) and np.array_equal(out["lat"][b].view(np.uint32), batch[3][b].view(np.uint32))


# ---- the kernel's order on the host, under the sanitizers ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("symrefine") / "sym_refine_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "sym_refine_host_check.cpp"), "-o", exe], check=True)
    return exe


def run_host_check(exe, tmp_path, batch, ch):
    P, F = ch["P"], ch["F"]
    B, N = len(batch[3]), len(batch[1])
    cf, of = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(cf, "wb") as f:
        f.write(struct.pack("<ii", B, N))
        for arr, dt in ((P["offsets"], np.int32), (P["info"], np.int32), (P["lat"], np.float64), (P["frac"], np.float64), (P["perm"], np.int32),
                        (P["spec_off"], np.int32), (batch[2], np.float32), (batch[3], np.float32), (F["info"], np.int32), (F["rot"], np.int32),
                        (F["trans"], np.float64)):
            f.write(np.ascontiguousarray(np.asarray(arr, dt)).tobytes())
    r = subprocess.run([exe, cf, of], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(of, "rb").read()
    out, pos = {}, 0
    for name, shape, dt in (("info", (B, 8), np.int32), ("stat", (B, 4), np.float64), ("orbit", (N,), np.int32), ("mult", (N,), np.int32),
                            ("site_order", (N,), np.int32), ("trans_ref", (B, S.MAX_OPS, 3), np.float64), ("frac", (N, 3), np.float32), ("lat", (B, 9), np.float32)):
        size = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[name] = np.frombuffer(raw[pos:pos + size], dt).reshape(shape)
        pos += size
    assert pos == len(raw)
    return out


def assert_equal_bits(got, ref):
    for k in V.KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_host_check_equals_the_restatement(host_check, tmp_path):
    names, batch, ch = RC.regular_results(POISON)
    assert_equal_bits(run_host_check(host_check, tmp_path, batch, ch), ch["ref"])


def test_host_check_equals_the_restatement_on_the_guards(host_check, tmp_path):
    batch, ch = RC.guard_results(POISON)
    assert_equal_bits(run_host_check(host_check, tmp_path, batch, ch), ch["ref"])


def test_header_table_constants_and_the_unit():
    from matinvent_amd import _lib, symmetry
    from matinvent_amd.build import ALL_SOURCES, MORE_SOURCES, SOURCES
    from tests.header_util import declared_symbols
    names = declared_symbols("matinvent_hip_sym_refine.h")
    assert names == ["mi_sym_refine"] and sorted(_lib.SYM_REFINE_SIGNATURES) == names
    assert any(t is _lib.SYM_REFINE_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    assert "sym_refine.hip" in MORE_SOURCES and "sym_refine.hip" in ALL_SOURCES and len(SOURCES) == 31 and len(set(ALL_SOURCES)) == len(ALL_SOURCES)
    head = open(os.path.join(ROOT, "include", "matinvent_hip_sym_refine.h")).read()
    ops = open(os.path.join(ROOT, "matinvent_amd", "csrc", "sym_refine.h")).read()
    unit = open(os.path.join(ROOT, "matinvent_amd", "csrc", "sym_refine.hip")).read()
    assert "#define MI_SYM_REFINE_FAIL 1024\n" in head and "SYM_REFINE_FAIL = 1024" in ops and _lib.SYM_REFINE_FAIL == V.REFINE_FAIL == 1024
    assert '#include "matinvent_hip_sym.h"' in head
    for other in ("matinvent_hip_sym.h", "matinvent_hip_sym_conv.h"):
        assert "MI_SYM_REFINE" not in open(os.path.join(ROOT, "include", other)).read()
    assert '#include "sym_ops.h"' in ops and "fp contract(off)" in ops and '#include "sym_refine.h"' in unit and "__launch_bounds__(SM_THREADS)" in unit
    for word in ("atomic", "mfma", "asm", "pow(", "cbrt", "exp(", "log(", "sin(", "cos(", "fma("):   # + - x /, sqrt and floor only; plain C++
        assert word not in ops, word
    for word in ("atomic", "mfma", "asm"):
        assert word not in unit.split("namespace mi {", 1)[1], word
    assert (_lib.SYM_REFINE_INFO, _lib.SYM_REFINE_STAT) == (V.NINFO, V.NSTAT) == (8, 4) and "REFINE_INFO = 8" in ops and "REFINE_STAT = 4" in ops
    assert symmetry.REFINE_INFO == V.INFO and [f[0] for f in _lib.SymRefineArgs._fields_][:4] == ["set", "types", "frac", "lat"]
    assert [f[0] for f in _lib.SymRefineArgs._fields_][4:] == ["sym_info", "sym_rot", "sym_trans", "out_frac", "out_lat", "orbit", "mult", "site_order", "trans_ref",
                                                                "refine_info", "refine_stat"]
    order = [head.index(" " + f[0] + ";") for f in _lib.SymRefineArgs._fields_]   # the struct's members in the table's order
    assert order == sorted(order)
    text = open(os.path.join(ROOT, "dropin", "configs", "reward", "symmetry_orbits.yaml")).read()
    assert "_target_: rewards.calculators.Symmetry" in text and "quantity: n_orbits" in text
    assert "n_orbits" not in open(os.path.join(ROOT, "dropin", "configs", "reward", "symmetry.yaml")).read()


# ---- the host module with the C calls replaced by the restatement ----------------------------------------------------------------------------------
class FakePrepared:
    def __init__(self, P, offsets, N):
        self.P, self.offsets, self.B, self.N, self.lat = P, offsets, len(P["info"]), N, torch.zeros(1)


class FakeSym:
    def __init__(self, F, tol):
        self.F, self.tol, self.info = F, tol, torch.from_numpy(np.ascontiguousarray(F["info"]))


@pytest.fixture
def stubbed(monkeypatch):
    """matinvent_amd.symmetry with prepare, find, primitive, conventional and refine computed by the restatements on CPU tensors; the
    stage logic of refine_arrays, refined_records and the reward run as they are."""
    from matinvent_amd import matching, symmetry
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    calls = []

    def prepare_arrays(offsets, types, frac, lat, fill=None):
        return FakePrepared(R.prepare(offsets.numpy(), types.numpy(), frac.numpy(), lat.numpy().reshape(-1, 9)), offsets, len(types))

    def find(prepared, tol, angle_tol=5.0, fill=None):
        tol = np.asarray(tol, np.float64)
        return FakeSym(S.find(prepared.P, tol, K.COS_TOL, margin=False), tol)

    def refine_prepared(prepared, types, frac, lat, sym, fill=None):
        calls.append("refine")
        r = V.refine(prepared.P, types.numpy(), frac.numpy(), lat.numpy(), sym.F)
        return symmetry.Refined(prepared.offsets, types, t(r["frac"]), t(r["lat"]), t(r["orbit"]), t(r["mult"]), t(r["site_order"]), t(r["trans_ref"]), t(r["info"]),
                                t(r["stat"]), sym.tol)

    def reduce_arrays(offsets, types, frac, lat, tol, angle_tol=5.0):
        calls.append("primitive")
        P = R.prepare(offsets.numpy(), types.numpy(), frac.numpy(), lat.numpy())
        F = S.find(P, np.asarray(tol), K.COS_TOL, margin=False)
        p = S.primitive(P, types.numpy(), frac.numpy(), lat.numpy(), F, margin=False)
        return symmetry.Primitive(t(p["prim_offsets"]), t(p["types"]), t(p["frac"]), t(p["lat"]), t(p["prim_count"]), t(p["prim_status"]), t(p["prim_det"])), FakeSym(F, tol)

    def conventional_arrays(offsets, types, frac, lat, tol, angle_tol=5.0):
        calls.append("conventional")
        ch = CV.chain((offsets.numpy(), types.numpy(), frac.numpy(), lat.numpy()), RC.SYMPREC, K.COS_TOL)
        c = ch["conv"]
        return symmetry.Conventional(t(c["conv_info"]), t(c["conv_M"]), t(c["conv_cvec"]), t(c["conv_count"]), t(c["conv_offsets"]), t(c["types"]), t(c["frac"]),
                                     t(c["lat"])), FakeSym(ch["F2"], tol)

    monkeypatch.setattr(matching, "prepare_arrays", prepare_arrays)
    for name, fn in (("find_symmetry_prepared", find), ("refine_prepared", refine_prepared), ("reduce_arrays", reduce_arrays), ("conventional_arrays", conventional_arrays)):
        monkeypatch.setattr(symmetry, name, fn)
    return symmetry, calls


def record(crystal):
    from matinvent_amd.data import SimpleStructure
    p = V.cell_parameters(crystal[0])
    return SimpleStructure(p[:3], p[3:], list(crystal[1]), np.asarray(crystal[2], np.float64))


def big_conventional():
    """Fm-3m in its primitive cell with 17 atoms -- the origin and the (x, x, x) orbits of x = 0.15 and x = 0.35, eight atoms each: its
    conventional cell has 68 atoms, more than the guard takes."""
    prim = K.FCC * 2.0
    z, f = [29], [np.zeros(3)]
    for species, x in ((8, 0.15), (16, 0.35)):
        pts = []
        for q in RC.orbit_of((x, x, x)):
            g = ((q * 8.0) @ np.linalg.inv(prim)) % 1.0
            g = np.where(np.abs(g - 1.0) < 1e-9, 0.0, g)
            if not any(np.abs((g - p) - np.round(g - p)).max() < 1e-9 for p in pts):
                pts.append(g)
        assert len(pts) == 8
        z += [species] * 8
        f += pts
    return prim, z, np.array(f)


@pytest.mark.parametrize("cell", ["given", "primitive", "conventional"])
def test_refine_arrays_stage_by_stage(stubbed, cell):
    symmetry, calls = stubbed
    p = RC.perturbed()
    crystals = [p["rutile"], p["rocksalt_conv"], K.cell("rocksalt_prim"), RC.AMBIGUOUS_CRYSTAL, p["hcp"]]
    batch = K.batch(crystals)
    tol = S.tolerances(batch[0], batch[3], RC.SYMPREC)
    got = symmetry.refine_arrays(*(torch.from_numpy(a) for a in batch), tol, cell=cell)
    want = V.chain_cell(batch, RC.SYMPREC, K.COS_TOL, cell)
    assert calls == ([] if cell == "given" else [cell]) + ["refine"]
    total = int(want["offsets"][-1])
    assert np.array_equal(got.offsets.numpy(), want["offsets"]) and np.array_equal(got.types.numpy()[:total], want["types"][:total])
    for k in ("frac", "orbit", "mult", "site_order"):
        assert np.array_equal(getattr(got, k).numpy()[:total], want[k][:total]), k
    for k in ("lat", "info", "stat"):
        assert np.array_equal(getattr(got, k).numpy(), want[k]), k
    atoms = {"given": [6, 8, 2, 2, 2], "primitive": [6, 2, 2, 2, 2], "conventional": [6, 8, 8, 2, 2]}[cell]
    assert np.diff(want["offsets"]).tolist() == atoms and (want["info"][[0, 1, 2, 4], 7] == S.OK).all() and want["info"][3, 7] & V.REFINE_FAIL
    assert want["info"][:3, 0].tolist() == [2, 2, 2]


def test_a_conventional_cell_beyond_the_guard_comes_back_as_the_stage_before_made_it(stubbed):
    symmetry, _ = stubbed
    batch = K.batch([big_conventional(), RC.perturbed()["rutile"]])
    tol = S.tolerances(batch[0], batch[3], RC.SYMPREC)
    got = symmetry.refine_arrays(*(torch.from_numpy(a) for a in batch), tol, cell="conventional")
    conv = CV.chain(batch, RC.SYMPREC, K.COS_TOL)["conv"]
    assert int(conv["conv_offsets"][1]) == 68 and conv["conv_info"][0, 7] == S.OK
    info = got.info.numpy()
    assert info[0, 7] & V.REFINE_FAIL and info[0, 7] & S.NOT_PREPARED and info[1].tolist() == [2, 16, 0, 0, 0, 0, 0, S.OK]
    assert np.array_equal(got.frac.numpy()[:68], conv["frac"][:68]) and np.array_equal(got.lat.numpy()[0], conv["lat"][0])
    assert got.orbit.numpy()[:68].tolist() == list(range(68)) and (got.mult.numpy()[:68] == 1).all() and (got.site_order.numpy()[:68] == 1).all()
    assert got.orbit.numpy()[68:74].tolist() == [0, 0, 2, 2, 2, 2]


def test_refined_records_and_the_result(stubbed):
    symmetry, _ = stubbed
    p = RC.perturbed()
    amb, tri = record(RC.AMBIGUOUS_CRYSTAL), record(C.known_crystals()["triclinic"][0])
    recs = [record(p["rutile"]), amb, tri, record(p["rocksalt_conv"])]
    out, res = symmetry.refined_records(recs, device="cpu")
    assert len(out) == 4 and len(res) == 4 and out[1] is amb and out[0] is not recs[0]
    assert res.status[[0, 2, 3]].tolist() == [0, 0, 0] and res.status[1] & V.REFINE_FAIL and res.n_orbits.tolist() == [2, 2, 3, 2] and res.n_ops.tolist()[0] == 16
    assert res.orbits(0).tolist() == [0, 0, 2, 2, 2, 2] and res.multiplicity(0).tolist() == [2, 2, 4, 4, 4, 4] and res.site_symmetry_order(0).tolist() == [8, 8, 4, 4, 4, 4]
    assert res.orbits(1).tolist() == [0, 1] and res.multiplicity(1).tolist() == [1, 1] and res.orbits(2).tolist() == [0, 1, 2] and len(res.orbits(3)) == 8
    assert 0 < res.rms_move[0] <= res.max_move[0] <= 2 * RC.MOVE and res.max_residual[0] <= 4 * RC.MOVE and res.max_move[1] == 0 and res.max_move[2] == 0
    assert 0 < res.cell_change[0] < 4 * RC.STRAIN and res.cell_change[2] == 0
    a, b, c, al, be, ga = res.cell_parameters[0]
    assert abs(a / b - 1) < 1e-6 and abs(a / c - 1) > 0.1 and max(abs(al - 90), abs(be - 90), abs(ga - 90)) < 1e-4
    assert np.allclose(out[0].lengths, [a, b, c]) and sorted(out[0].species) == sorted(recs[0].species)
    # the same numbers as the restatement's, in A
    batch = K.batch([p["rutile"]])
    ch = V.chain(batch, RC.SYMPREC, K.COS_TOL)
    scale = RC.SYMPREC / ch["tol"][0]
    assert np.isclose(res.max_move[0], ch["ref"]["stat"][0, 0] * scale, rtol=1e-5) and np.isclose(res.rms_move[0], ch["ref"]["stat"][0, 1] * scale, rtol=1e-5)
    prim, pres = symmetry.symmetry_primitive_records([recs[3]], device="cpu")
    assert len(prim[0].species) == 2 and pres.n_ops.tolist() == [48] and pres.n_orbits.tolist() == [2]
    empty = symmetry.refined_records([], device="cpu")
    assert empty[0] == [] and len(empty[1]) == 0


def test_an_unknown_cell_is_refused():
    from matinvent_amd import symmetry
    with pytest.raises(ValueError, match="none of"):
        symmetry.refine_arrays(None, None, None, None, None, cell="standard")
    with pytest.raises(ValueError, match="none of"):
        symmetry.refined_records([1], cell="refined")


def test_the_reward_quantities(stubbed):
    from matinvent_amd import rewards
    p = RC.perturbed()
    recs = [record(C.known_crystals()["rutile"][0]), record(RC.AMBIGUOUS_CRYSTAL), record(p["rutile"])]
    out = rewards.Symmetry(quantity="n_orbits", device="cpu").calc((recs, None))
    assert out[0] == 2.0 and np.isnan(out[1]) and out[2] == 2.0
    d = rewards.Symmetry(quantity="distortion", device="cpu").calc(recs)
    assert d[0] < 1e-6 and np.isnan(d[1]) and 1e-3 < d[2] <= RC.MOVE
    for q in ("n_orbits", "distortion"):
        assert q in rewards.Symmetry.QUANTITIES and rewards.Symmetry(q).calc([]).shape == (0,)
    assert rewards.Symmetry.QUANTITIES[:6] == ("n_ops", "pg_order", "not_p1", "crystal_system", "bravais", "centring_mult")
    with pytest.raises(ValueError, match="none of"):
        rewards.Symmetry(quantity="wyckoff")
