"""GPU: every output of mi_sm_prepare and mi_sm_match equals the numpy restatement tests/sm_ref64.py bit for bit -- the
reduced cells and sorted coordinates, the map list in order, rms and max_dist, the best map and translation, the permutation, the counts
and the status -- on both LDS tiles, behind the guards with poisoned outputs, and wherever a pair stands in its list."""
import numpy as np
import pytest
import torch

from tests import sm_cases as K
from tests import sm_ref64 as R
from tests.test_struct_match_host import guard_batch, known_displacement, regular

pytestmark = pytest.mark.gpu

POISON = -7


def poison(shape, dt):
    return torch.full(shape, POISON, dtype=dt, device="cuda")


def device_prepare(off, types, frac, lat, fill=None):
    from matinvent_amd import matching
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return matching.prepare_arrays(t(off), t(types), t(frac), t(lat), fill)


def assert_prepared_equal(S, P):
    for k in ("lat", "inv", "frac", "types", "perm", "spec_Z", "spec_off", "info"):
        got = getattr(S, k).cpu().numpy()
        assert np.array_equal(got[:len(P[k])], P[k]), k


def assert_pairs_equal(out, res):
    host = {k: v.cpu().numpy() for k, v in out.items()}
    for p, r in enumerate(res):
        assert host["status"][p] == r["status"], p
        assert host["rms"][p] == r["rms"] and host["max_dist"][p] == r["max_dist"], (p, host["rms"][p], r["rms"])
        assert list(host["best_map"][p]) == list(r["best_map"]) and host["best_trans"][p] == r["best_trans"], p
        assert host["n_maps"][p] == r["n_maps"] and host["n_items"][p] == r["n_items"], p
        if "perm" in host:
            assert list(host["perm"][p]) == list(r["perm"]), p
        if "maps" in host and r["status"] == R.OK:
            assert host["maps"][p][:r["n_maps"]].tolist() == r["maps"], p


@pytest.fixture(scope="module")
def regular_device():
    from matinvent_amd import matching
    crystals, pairs, P, res = regular()
    S = device_prepare(*K.batch(crystals))
    out = matching.match_pairs(S, S, pairs, permutation=True, maps=True, fill=poison)
    return S, out


def test_prepare_and_match_equal_the_restatement(regular_device):
    """1, 2, 3, 8, 20 (3 species, the rarest 4), 33 and 64 atoms; the named cells, where all 48 (24) maps tie and the lowest item wins."""
    crystals, pairs, P, res = regular()
    S, out = regular_device
    assert_prepared_equal(S, P)
    assert_pairs_equal(out, res)
    assert int(out["best_trans"][pairs.index((8, 8))]) == 0 and out["best_map"][pairs.index((8, 8))].tolist() == res[pairs.index((8, 8))]["maps"][0]


def test_both_tiles_give_the_same_bits(regular_device):
    from matinvent_amd import matching
    crystals, pairs, P, res = regular()
    S, out = regular_device
    big = matching.match_pairs(S, S, pairs, permutation=True, maps=True, large_tile=True, fill=poison)
    for k in out:
        assert torch.equal(out[k], big[k]), k


def test_a_pair_does_not_depend_on_its_list(regular_device):
    """300 pairs of 1 .. 3-atom crystals; one query against 300 candidates; a pair alone against itself at positions 0, 150 and 299."""
    from matinvent_amd import matching
    crystals, pairs, P, res = regular()
    S, out = regular_device
    small = [p for p in pairs if P["info"][p[0], 0] <= 3]
    lst = [small[i % len(small)] for i in range(300)]
    probe = pairs[pairs.index((20, 21))]
    for pos in (0, 150, 299):
        lst[pos] = probe
    many = matching.match_pairs(S, S, lst, permutation=True)
    alone = matching.match_pairs(S, S, [probe], permutation=True)
    for k in alone:
        for pos in (0, 150, 299):
            assert torch.equal(many[k][pos], alone[k][0]), (k, pos)
    for i in (1, 2, 151, 298):
        j = pairs.index(lst[i])
        assert float(many["rms"][i]) == res[j]["rms"] and many["perm"][i].tolist() == res[j]["perm"]
    one = matching.match_pairs(S, S, [(6, c % len(crystals)) for c in range(300)])
    again = matching.match_pairs(S, S, [(6, 7)])
    assert torch.equal(one["rms"][7], again["rms"][0]) and int(one["status"][7 + len(crystals)]) == int(again["status"][0])


def test_guards_keep_their_status_and_the_rest_of_the_batch():
    from matinvent_amd import matching
    off, types, frac, lat, pairs = guard_batch()
    B, N = len(off) - 1, len(types)
    fill = {"lat": np.full((B, 9), float(POISON)), "inv": np.full((B, 9), float(POISON)), "frac": np.full((N, 3), float(POISON)),
            "types": np.full(N, POISON, np.int32), "perm": np.full(N, POISON, np.int32), "spec_Z": np.full((B, 16), POISON, np.int32),
            "spec_off": np.full((B, 17), POISON, np.int32), "info": np.full((B, 4), POISON, np.int32)}
    P = R.prepare(off, types, frac, lat, fill=fill)
    S = device_prepare(off, types, frac, lat, fill=poison)
    assert_prepared_equal(S, P)
    res = [R.match_pair(P, q, P, c, 0.2, K.COS_TOL) for q, c in pairs]
    out = matching.match_pairs(S, S, pairs, permutation=True, fill=poison)
    assert_pairs_equal(out, res)
    assert sorted(set(int(s) for s in out["status"])) == [R.OK, R.SPECIES_MISMATCH, R.BAD_PAIR, R.NOT_PREPARED]


def test_known_displacement_within_four_units():
    """The device against mpmath on the 20-atom known displacement, within 4 x the restatement's own deviation (measured: the device equals
    the restatement bit for bit, so 1 x)."""
    import mpmath as mp
    from matinvent_amd import matching
    crystals, exact = known_displacement()
    P = R.prepare(*K.batch(crystals))
    unit = abs(mp.mpf(R.match_pair(P, 0, P, 1, 0.2, K.COS_TOL)["rms"]) - exact)
    S = device_prepare(*K.batch(crystals))
    out = matching.match_pairs(S, S, [(0, 1)], permutation=True)
    dev = abs(mp.mpf(float(out["rms"][0])) - exact)
    print("device deviation", mp.nstr(dev, 5), "restatement deviation", mp.nstr(unit, 5))
    assert dev <= 4 * unit
    assert out["perm"][0, :20].tolist() == list(range(20))
