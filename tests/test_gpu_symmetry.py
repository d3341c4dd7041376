"""GPU: every output of mi_sym_find and mi_sym_primitive equals the numpy restatement tests/sym_ref64.py bit for bit -- the
counts, rot, trans, dev, ptrans, the histogram, the indices, the status, and the primitive frac / lat / types / prim_offsets -- on poisoned
output buffers, behind the guards, and wherever a crystal stands in its batch."""
import numpy as np
import pytest
import torch

from tests import sm_cases as K
from tests import sm_ref64 as R
from tests import sym_cases as C
from tests import sym_ref64 as S
from tests.test_struct_match_host import guard_batch

pytestmark = pytest.mark.gpu

POISON = -7
FIND_KEYS = ("info", "rot_hist", "rot", "trans", "dev", "ptrans")


def poison(shape, dt):
    return torch.full(shape, POISON, dtype=dt, device="cuda")


def device_run(off, types, frac, lat, tol, fill=poison):
    """(find arrays, primitive arrays) of the device as numpy dicts with the restatement's keys."""
    from matinvent_amd import matching, symmetry
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_off, d_types, d_frac, d_lat = t(off), t(types), t(frac), t(lat)
    prepared = matching.prepare_arrays(d_off, d_types, d_frac, d_lat)
    sym = symmetry.find_symmetry_prepared(prepared, tol, fill=fill)
    prim = symmetry.primitive_arrays(prepared, d_types, d_frac, d_lat, sym, fill=fill)
    F = {k: getattr(sym, k).cpu().numpy() for k in FIND_KEYS}
    Pm = {"prim_offsets": prim.offsets, "types": prim.types, "frac": prim.frac, "lat": prim.lat, "prim_count": prim.count, "prim_status": prim.status,
          "prim_det": prim.det}
    return F, {k: v.cpu().numpy()[:len(types)] if k in ("types", "frac") else v.cpu().numpy() for k, v in Pm.items()}


def assert_equal_bits(got_f, got_p, F, prim):
    for k in FIND_KEYS:
        assert np.array_equal(got_f[k], F[k]), k
    for k in ("prim_count", "prim_status", "prim_det", "prim_offsets", "types", "frac", "lat"):
        assert np.array_equal(got_p[k], prim[k], equal_nan=True), k


def test_known_and_random_crystals_equal_the_restatement():
    """The known crystals (1 .. 8 atoms; 192 operations on rock salt) and random ones of 1, 2, 3, 8, 20 (three species, the rarest 4), 33
    and 64 atoms: both sides of the wave width."""
    crystals = [v[0] for v in C.known_crystals().values()] + C.random_set()
    batch, P, tol, F, prim = C.analyse(crystals, fill=POISON)
    got_f, got_p = device_run(*batch, tol)
    assert_equal_bits(got_f, got_p, F, prim)
    assert F["info"][5].tolist()[:2] == [192, 4] and (F["info"][:, 7] == S.OK).sum() >= len(crystals) - 1


def test_capped_supercell_equals_the_restatement():
    batch, P, tol, F, _ = C.capped_results()
    prim = S.primitive(P, batch[1], batch[2], batch[3], F, fill=POISON)
    got_f, got_p = device_run(*batch, tol)
    assert_equal_bits(got_f, got_p, F, prim)   # (every one of the 192 and 64 rows of the find arrays is written, so their fill does not show)
    assert got_f["info"][0].tolist() == [3072, 64, 48, 48, 32, 7, 1, S.OPS_CAP] and got_p["prim_offsets"].tolist() == [0, 1]


def test_a_crystal_does_not_depend_on_its_batch():
    """300 crystals of 1 .. 3 atoms; rock salt at positions 0, 150 and 299 equals rock salt on its own."""
    rng = np.random.default_rng(61)
    small = [K.random_crystal(rng, c) for c in ([1], [2], [1, 2])]
    rock = K.cell("rocksalt_conv")
    crystals = [small[i % 3] for i in range(300)]
    for pos in (0, 150, 299):
        crystals[pos] = rock
    from matinvent_amd import matching, symmetry
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def run(cs):
        off, types, frac, lat = K.batch(cs)
        tol = S.tolerances(off, lat, C.SYMPREC)
        args = (t(off), t(types), t(frac), t(lat))
        prepared = matching.prepare_arrays(*args)
        sym = symmetry.find_symmetry_prepared(prepared, tol, fill=poison)
        return sym, symmetry.primitive_arrays(prepared, *args[1:], sym, fill=poison)

    many, many_p = run(crystals)
    alone, alone_p = run([rock])
    for pos in (0, 150, 299):
        for k in FIND_KEYS:
            assert torch.equal(getattr(many, k)[pos], getattr(alone, k)[0]), (k, pos)
        lo, hi = int(many_p.offsets[pos]), int(many_p.offsets[pos + 1])
        assert hi - lo == 2 and torch.equal(many_p.types[lo:hi], alone_p.types[:2]) and torch.equal(many_p.frac[lo:hi], alone_p.frac[:2])
        assert torch.equal(many_p.lat[pos], alone_p.lat[0]) and torch.equal(many_p.det[pos], alone_p.det[0])
    assert many.n_ops[1] >= 1 and int(many_p.offsets[-1]) == sum(len(c[1]) for c in crystals) - 3 * 6


def test_guards_keep_their_status_and_the_rest_of_the_batch():
    off, types, frac, lat, _ = guard_batch()
    P = R.prepare(off, types, frac, lat)
    tol = S.tolerances(np.clip(off, 0, len(types)), lat, C.SYMPREC)
    F = S.find(P, tol, K.COS_TOL, fill=POISON)
    prim = S.primitive(P, types, frac, lat, F, fill=POISON)
    got_f, got_p = device_run(off, types, frac, lat, tol)
    assert_equal_bits(got_f, got_p, F, prim)
    flagged = [b for b in range(len(lat)) if P["info"][b][3] != R.PREP_OK]
    assert len(flagged) == 7
    for b in flagged:
        assert got_f["info"][b].tolist() == [0] * 7 + [S.NOT_PREPARED] and (got_f["rot"][b] == POISON).all() and (got_f["dev"][b] == POISON).all()
    assert (got_f["info"][[0, 5, 9], 7] == S.OK).all()
