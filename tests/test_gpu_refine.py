"""GPU: every output of mi_sym_refine equals the numpy restatement tests/refine_ref64.py bit for bit -- both info arrays, the
orbits, multiplicities and site orders, the refined translations, the float32 coordinates and cells -- on poisoned output buffers, behind
the guards, and wherever a crystal stands in its batch.  The chain in front of the entry (prepare, find) is the device's own, which
tests/test_gpu_symmetry.py holds to the same restatement."""
import numpy as np
import pytest
import torch

from tests import refine_cases as RC
from tests import refine_ref64 as V
from tests import sm_cases as K
from tests import sm_ref64 as R
from tests import sym_ref64 as S

pytestmark = pytest.mark.gpu

POISON = -7


def poison(shape, dt):
    return torch.full(shape, POISON, dtype=dt, device="cuda")


def device_chain(off, types, frac, lat, tol, fill=poison):
    """(Refined, SymmetryResult) with the entry's outputs built by `fill`."""
    from matinvent_amd import matching, symmetry
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    off, types, frac, lat = t(off), t(types), t(frac), t(lat)
    prepared = matching.prepare_arrays(off, types, frac, lat)
    sym = symmetry.find_symmetry_prepared(prepared, tol)
    return symmetry.refine_prepared(prepared, types, frac, lat, sym, fill=fill), sym


def as_numpy(ref, N):
    got = {"info": ref.info, "stat": ref.stat, "orbit": ref.orbit, "mult": ref.mult, "site_order": ref.site_order, "trans_ref": ref.trans_ref, "frac": ref.frac,
           "lat": ref.lat}
    return {k: v.cpu().numpy()[:N] if k in ("orbit", "mult", "site_order", "frac") else v.cpu().numpy() for k, v in got.items()}


def assert_equal_bits(got, ref):
    for k in V.KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a.reshape(len(a), -1).view(np.uint8) != b.reshape(len(b), -1).view(np.uint8))[:, 0]
            raise AssertionError((k, sorted(set(int(v) for v in bad))[:8]))


def test_known_perturbed_and_random_crystals_equal_the_restatement():
    """The known crystals (rocksalt_conv: 192 operations, every operation thread live), the 64-atom Pm-3m cell (every atom thread of a wave
    live), a one-atom cube (48 operations, one atom), the perturbed crystals and their transformed copies, and P1 crystals of 1, 2, 3, 8,
    20, 33 and 64 atoms (the copy path)."""
    names, batch, ch = RC.regular_results(POISON)
    ref, _ = device_chain(*batch, ch["tol"])
    got = as_numpy(ref, len(batch[1]))
    assert_equal_bits(got, ch["ref"])
    info = dict(zip(names, got["info"]))
    assert info["rocksalt_conv"].tolist() == [2, 192, 0, 0, 0, 0, 0, S.OK] and info["pm3m_64~"].tolist() == [4, 48, 0, 0, 0, 0, 0, S.OK]
    assert info["one_atom_cubic"].tolist() == [1, 48, 0, 0, 0, 0, 0, S.OK] and info["random6"].tolist() == [64, 1, 0, 0, 0, 0, 0, S.OK]
    assert sum(1 for r in got["info"] if r[1] > 1 and r[7] == S.OK) >= 22 and (got["stat"][[names.index(n + "~") for n in RC.PERTURBED], 1] > 0).all()


def test_guards_copy_or_write_nothing_and_keep_the_rest_of_the_batch():
    batch, ch = RC.guard_results(POISON)
    ref, sym = device_chain(*batch, ch["tol"])
    got = as_numpy(ref, len(batch[1]))
    assert_equal_bits(got, ch["ref"])
    assert got["info"][[0, 5], :2].tolist() == [[2, 16], [2, 192]] and (got["info"][[0, 5], 7] == S.OK).all()
    for b in (1, 2):   # a NaN lattice, a flat cell: the info row and nothing else
        lo, hi = int(batch[0][b]), int(batch[0][b + 1])
        assert got["info"][b, 7] == S.NOT_PREPARED | V.REFINE_FAIL and (got["frac"][lo:hi] == POISON).all() and (got["lat"][b] == POISON).all()
    for b in (3, 4):   # more operations than the cap, an ambiguous crystal: copied, bit for bit
        lo, hi = int(batch[0][b]), int(batch[0][b + 1])
        assert got["info"][b, 7] == int(sym.info[b, 7]) | V.REFINE_FAIL and got["info"][b, 0] == hi - lo
        assert np.array_equal(got["frac"][lo:hi].view(np.uint32), batch[2][lo:hi].view(np.uint32)) and np.array_equal(got["lat"][b].view(np.uint32), batch[3][b].view(np.uint32))
        assert got["orbit"][lo:hi].tolist() == list(range(hi - lo)) and (got["mult"][lo:hi] == 1).all() and (got["site_order"][lo:hi] == 1).all()
    assert int(sym.info[3, 7]) == S.OPS_CAP and int(sym.info[4, 7]) & S.AMBIGUOUS


def test_refine_arrays_returns_every_guard_crystal_as_it_came():
    """Through refine_arrays the crystals the prepare guard rejected come back unchanged as well, bit for bit, with the fail bit and one
    orbit per atom."""
    from matinvent_amd import symmetry
    batch, ch = RC.guard_results(POISON)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ref = symmetry.refine_arrays(t(batch[0]), t(batch[1]), t(batch[2]), t(batch[3]), ch["tol"])
    want = V.chain_cell(batch, RC.SYMPREC, K.COS_TOL, "given")
    N = len(batch[1])
    for k in ("frac", "orbit", "mult", "site_order"):
        assert np.array_equal(getattr(ref, k).cpu().numpy()[:N], want[k], equal_nan=True), k
    for k in ("lat", "info", "stat"):
        assert np.array_equal(getattr(ref, k).cpu().numpy(), want[k], equal_nan=True), k
    for b in (1, 2, 3, 4):
        lo, hi = int(batch[0][b]), int(batch[0][b + 1])
        assert int(ref.info[b, 7]) & V.REFINE_FAIL and ref.orbit[lo:hi].tolist() == list(range(hi - lo))
        assert np.array_equal(ref.frac[lo:hi].cpu().numpy().view(np.uint32), batch[2][lo:hi].view(np.uint32))
        assert np.array_equal(ref.lat[b].cpu().numpy().view(np.uint32), batch[3][b].view(np.uint32))


def test_a_crystal_does_not_depend_on_its_batch():
    """300 crystals of 1 .. 3 atoms; perturbed rock salt at positions 0, 150 and 299 equals perturbed rock salt on its own, which equals
    the restatement."""
    crystals = RC.batch_300()

    def run(cs):
        off, types, frac, lat = K.batch(cs)
        return device_chain(off, types, frac, lat, S.tolerances(off, lat, RC.SYMPREC))[0], off

    (many, off), (alone, _) = run(crystals), run([crystals[0]])
    names, batch, ch = RC.regular_results(POISON)
    b = names.index("rocksalt_conv~")
    lo = int(batch[0][b])
    want = ch["ref"]
    assert alone.info[0].tolist() == [2, 192, 0, 0, 0, 0, 0, S.OK]
    assert np.array_equal(alone.frac.cpu().numpy(), want["frac"][lo:lo + 8]) and np.array_equal(alone.trans_ref[0].cpu().numpy(), want["trans_ref"][b])
    assert np.array_equal(alone.stat[0].cpu().numpy(), want["stat"][b]) and np.array_equal(alone.lat[0].cpu().numpy(), want["lat"][b])
    for pos in (0, 150, 299):
        for k in ("info", "stat", "lat", "trans_ref"):
            assert torch.equal(getattr(many, k)[pos], getattr(alone, k)[0]), (k, pos)
        at = int(off[pos])
        for k in ("frac", "orbit", "mult", "site_order"):
            assert torch.equal(getattr(many, k)[at:at + 8], getattr(alone, k)[:8]), (k, pos)
    info = many.info.cpu().numpy()
    for r in (1, 2, 3):   # the small crystals repeat with period three
        rows = info[r:150:3]
        assert (rows == rows[0]).all() and rows[0, 7] != POISON
    assert (many.orbit.cpu().numpy() != POISON).all() and (many.frac.cpu().numpy() != POISON).all()
