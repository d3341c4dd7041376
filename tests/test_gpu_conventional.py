"""GPU: every output of mi_sym_conventional equals the numpy restatement tests/conv_ref64.py bit for bit -- the info row, M, the
centring vectors, the counts and offsets, types, float32 coordinates and cells -- on poisoned output buffers, behind the guards, and
wherever a crystal stands in its batch.  The chain in front of the entry (prepare, find, primitive, prepare, find) is the device's own,
which tests/test_gpu_symmetry.py holds to the same restatement."""
import numpy as np
import pytest
import torch

from tests import conv_cases as CC
from tests import conv_ref64 as V
from tests import sm_cases as K
from tests import sm_ref64 as R
from tests import sym_cases as C
from tests import sym_ref64 as S
from tests.test_conventional_host import status_batch

pytestmark = pytest.mark.gpu

POISON = -7
KEYS = ("conv_info", "conv_M", "conv_cvec", "conv_count", "conv_offsets", "types", "frac", "lat")


def poison(shape, dt):
    return torch.full(shape, POISON, dtype=dt, device="cuda")


def device_chain(off, types, frac, lat, tol, fill=poison):
    """(Conventional, SymmetryResult of the primitive crystals) with the entry's outputs built by `fill`."""
    from matinvent_amd import matching, symmetry
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    prim, _ = symmetry.reduce_arrays(t(off), t(types), t(frac), t(lat), tol)
    prepared = matching.prepare_arrays(prim.offsets, prim.types, prim.frac, prim.lat)
    sym = symmetry.find_symmetry_prepared(prepared, tol)
    return symmetry.conventional_prepared(prepared, prim.types, prim.frac, prim.lat, sym, fill=fill), sym


def as_numpy(conv, N):
    got = {"conv_info": conv.info, "conv_M": conv.M, "conv_cvec": conv.cvec, "conv_count": conv.count, "conv_offsets": conv.offsets, "types": conv.types,
           "frac": conv.frac, "lat": conv.lat}
    return {k: v.cpu().numpy()[:4 * N] if k in ("types", "frac") else v.cpu().numpy() for k, v in got.items()}


def assert_equal_bits(got, ref):
    for k in KEYS:
        assert np.array_equal(got[k], ref[k], equal_nan=True), k


def test_fixtures_and_random_crystals_equal_the_restatement():
    """The 14 lattices and the lower-symmetry crystals as typed and transformed, the known crystals, and P1 crystals of 1, 2, 3, 8, 20, 33
    and 64 atoms (M = I, mult 1)."""
    cases = CC.all_cases()
    crystals = [c[1] for c in cases] + C.random_set()
    batch = K.batch(crystals)
    ch = V.chain(batch, CC.SYMPREC, K.COS_TOL, fill=POISON)
    conv, _ = device_chain(*batch, ch["tol"])
    got = as_numpy(conv, len(batch[1]))
    assert_equal_bits(got, ch["conv"])
    assert set(got["conv_info"][:len(cases), 0].tolist()) == set(range(1, 15)) and (got["conv_info"][:len(cases), 7] == S.OK).all()
    rand = got["conv_info"][len(cases):]
    ok = rand[:, 7] == S.OK   # (the one-atom random crystal's operations are not a group for the finder: it comes back as it was)
    assert ok.sum() >= len(rand) - 1 and (rand[ok, :3] == [1, 1, 1]).all() and (rand[~ok, 0] == 0).all() and (rand[~ok, 7] & V.CONV_FAIL).all()
    assert (got["conv_M"][len(cases):] == V.IDENT).all()
    total = int(got["conv_offsets"][-1])
    assert (got["types"][total:] == POISON).all() and (got["frac"][total:] == POISON).all()


def test_a_crystal_does_not_depend_on_its_batch():
    """300 crystals of 1 .. 3 atoms; primitive rock salt at positions 0, 150 and 299 equals primitive rock salt on its own."""
    rng = np.random.default_rng(67)
    small = [K.random_crystal(rng, c) for c in ([1], [2], [1, 2])]
    rock = CC.rocksalt_prim()
    crystals = [small[i % 3] for i in range(300)]
    for pos in (0, 150, 299):
        crystals[pos] = rock

    def run(cs):
        off, types, frac, lat = K.batch(cs)
        return device_chain(off, types, frac, lat, S.tolerances(off, lat, CC.SYMPREC))[0]

    many, alone = run(crystals), run([rock])
    assert alone.info[0].tolist() == [14, V.F_, 4, 7, 3, int(alone.info[0, 5]), 0, S.OK] and int(alone.offsets[1]) == 8
    for pos in (0, 150, 299):
        for k in ("info", "M", "cvec", "count", "lat"):
            assert torch.equal(getattr(many, k)[pos], getattr(alone, k)[0]), (k, pos)
        lo, hi = int(many.offsets[pos]), int(many.offsets[pos + 1])
        assert hi - lo == 8 and torch.equal(many.types[lo:hi], alone.types[:8]) and torch.equal(many.frac[lo:hi], alone.frac[:8])
    assert int(many.offsets[-1]) == sum(len(c[1]) for c in crystals) + 3 * 6


def test_guards_write_nothing_and_keep_the_rest_of_the_batch():
    batch = status_batch()
    ch = V.chain(batch, CC.SYMPREC, K.COS_TOL, fill=POISON)
    conv, sym = device_chain(*batch, ch["tol"])
    got = as_numpy(conv, len(batch[1]))
    assert_equal_bits(got, ch["conv"])
    flagged = [b for b in range(len(batch[3])) if ch["P2"]["info"][b][3] != R.PREP_OK]
    assert len(flagged) == 7
    for b in flagged:
        assert got["conv_count"][b] == 0 and got["conv_info"][b, 0] == 0 and got["conv_info"][b, 7] & S.NOT_PREPARED and got["conv_info"][b, 7] & V.CONV_FAIL
        assert (got["lat"][b] == POISON).all() and got["conv_offsets"][b] == got["conv_offsets"][b + 1]
    assert got["conv_info"][1, 7] == int(sym.info[1, 7]) | V.CONV_FAIL and got["conv_info"][1, 7] & S.AMBIGUOUS and got["conv_count"][1] == 2
    assert got["conv_info"][[0, 2], 0].tolist() == [14, 14] and got["conv_count"][[0, 2]].tolist() == [8, 8]
