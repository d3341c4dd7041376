"""GPU: the substrate matcher (matinvent_amd.substrates) against the numpy restatement tests/zsl_ref64.py on poisoned output
buffers -- every integer (plane, n_f, n_s, HNFs, n_matches, status), every area, the plane vectors and the table lengths bit for bit;
theta and the strains to 4 x the restatement's own deviation from a higher-precision evaluation of the same formulas -- behind the guards,
wherever a film stands in its batch, and through match_records, primitive=True and the reward calculator."""

import numpy as np
import pytest
import torch

from tests import zsl_cases as Z
from tests import zsl_ref64 as R
from tests.test_zsl_host import compare

pytestmark = pytest.mark.gpu

POISON = -7


def poison(shape, dt):
    return torch.full(shape, POISON, dtype=dt, device="cuda")


def make_bank(bank, zsl, fill=poison):
    from matinvent_amd import substrates
    return substrates.SubstrateBank([substrates.Substrate(f"s{k}", lat.reshape(3, 3), hkls) for k, (lat, hkls) in enumerate(bank)], zsl, "cuda", fill=fill)


def device_run(films, m, bank, count, fill=poison):
    """The device's arrays as a numpy dict with the restatement's keys."""
    from matinvent_amd import substrates
    zsl = substrates.ZSL(film_max_miller=m)
    bk = make_bank(bank, zsl, fill)
    res = substrates.match_arrays(zsl, torch.from_numpy(np.ascontiguousarray(films, np.float32)).cuda(), bk, count, fill=fill)
    out = {k: getattr(bk, k).cpu().numpy() for k in ("vec", "area", "mult", "status")}
    out = {"s_" + k: v for k, v in out.items()}
    out["s_table"] = bk.table.cpu().numpy()
    out.update({"f_" + k: v.cpu().numpy() for k, v in zip(("vec", "area", "mult", "status"), res.planes)})
    out.update(res_d=res.res_d.cpu().numpy(), res_i=res.res_i.cpu().numpy(), res_n=res.res_n.cpu().numpy(), mcia=res.d_mcia.cpu().numpy(),
               mcia_plane=res.d_mcia_plane.cpu().numpy(), mcia_status=res.d_mcia_status.cpu().numpy())
    return out, res


@pytest.mark.parametrize("name", sorted(Z.CASES))
def test_cases_equal_the_restatement(name):
    """The closed forms, orthorhombic cells, 8 seeded triclinic cells, a hexagonal substrate with all 13 planes, a bank of 3 substrates,
    film_max_miller = 2, count mode on the three smallest cases, the tie between (001), (010) and (100) of a cubic film, and the guards
    (a NaN lattice, a flat cell, a cell so small that MULT_CAP fires) beside regular films that keep their bits."""
    films, m, bank, count = Z.CASES[name]
    got, _ = device_run(films, m, bank, count)
    ratios = compare(Z.reference(name), got, Z.deviation(name), name)
    print(f"TOL zsl device {name}: theta {ratios[0]:.2f} x, strains {ratios[1]:.2f} x the restatement's deviation")


def test_a_film_does_not_depend_on_its_batch():
    """300 films; one known film at positions 0, 150 and 299 equals that film alone (and the restatement), in count mode."""
    known = Z.ORTHO[0]
    rng = np.random.default_rng(7)
    films = np.stack([Z.cell(rng.uniform(5.0, 9.0, 3), rng.uniform(75.0, 105.0, 3)) for _ in range(300)])
    for pos in (0, 150, 299):
        films[pos] = known
    bank = [Z.SI_100, Z.TETRA]
    big, _ = device_run(films, 1, bank, True)
    alone, _ = device_run(known[None], 1, bank, True)
    for k in ("res_d", "res_i", "res_n", "mcia", "mcia_plane", "mcia_status"):
        for pos in (0, 150, 299):
            assert big[k][pos].tobytes() == alone[k][0].tobytes(), (k, pos)
    for k in ("f_vec", "f_area", "f_mult", "f_status"):
        for pos in (0, 150, 299):
            assert big[k].reshape(300, 13, -1)[pos].tobytes() == alone[k].tobytes(), (k, pos)
    ref = Z.reference("ortho_count")
    assert np.array_equal(alone["res_i"][0], ref["res_i"][0]) and np.array_equal(alone["res_n"][0], ref["res_n"][0]) and np.array_equal(alone["mcia"][0], ref["mcia"][0])
    assert not (big["res_d"] == POISON).any() and not (big["res_i"] == POISON).any() and not (big["res_n"] == POISON).any()


def test_chunks_of_films_equal_one_launch(monkeypatch):
    from matinvent_amd import substrates
    films, m, bank, count = Z.CASES["bank"]
    one, _ = device_run(films, m, bank, count)
    monkeypatch.setattr(substrates, "ITEM_CAP", 2 * 13 * 17)   # two films per search launch
    two, _ = device_run(films, m, bank, count)
    assert all(one[k].tobytes() == two[k].tobytes() for k in ("res_d", "res_i", "res_n", "mcia", "mcia_plane", "mcia_status"))


def test_match_records_primitive_and_the_saved_bank(tmp_path):
    from matinvent_amd import substrates, symmetry
    from matinvent_amd.data import SimpleStructure
    zsl = substrates.ZSL()
    bank = make_bank([Z.SI_100, Z.TETRA], zsl, fill=None)
    recs = [SimpleStructure([3.9, 5.6, 7.2], [90.0] * 3, [8], np.zeros((1, 3))), "not a crystal", SimpleStructure([4.1, 4.7, 9.3], [90.0] * 3, [8], np.zeros((1, 3)))]
    res = substrates.match_records(zsl, recs, bank)
    ref = Z.reference("ortho")
    assert len(res) == 3 and res.mcia_status[:, 0].tolist() == [R.OK, R.BAD_CELL, R.OK] and np.isinf(res.mcia[1]).all()
    for k, b in ((0, 0), (2, 1)):   # records equal the array entry
        assert np.array_equal(res.area[k], ref["res_d"][b, :, 0]) and np.array_equal(res.n_f[k], ref["res_i"][b, :, 2]) and np.array_equal(res.mcia[k], ref["mcia"][b])
        assert np.array_equal(res.film_hnf[k], ref["res_i"][b, :, 4:7]) and np.array_equal(res.sub_hnf[k], ref["res_i"][b, :, 7:10]) and (res.n_matches[k] == -1).all()
    # the saved bank holds data only and gives the same bits
    path = bank.save(str(tmp_path / "bank.npz"))
    with np.load(path, allow_pickle=False) as f:
        assert sorted(f.files) == sorted(("names", "max_area") + substrates.SubstrateBank.FIELDS)
    again = substrates.match_records(zsl, recs, substrates.SubstrateBank.load(path))
    assert again.res_d.cpu().numpy().tobytes() == res.res_d.cpu().numpy().tobytes() and again.res_i.cpu().numpy().tobytes() == res.res_i.cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="max_area"):
        substrates.match_records(substrates.ZSL(max_area=200.0), recs, bank)
    # primitive=True on conventional rock salt equals its primitive cell given directly
    a = 5.64
    pos = [[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5], [0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5], [0.5, 0.5, 0.5]]
    rock = SimpleStructure([a] * 3, [90.0] * 3, [11] * 4 + [17] * 4, np.array(pos, float))
    prim, ntr = symmetry.primitive_records([rock])
    assert ntr.tolist() == [4] and len(prim[0].species) == 2
    via, direct, conv = (substrates.match_records(zsl, r, bank, primitive=p) for r, p in (([rock], True), (prim, False), ([rock], False)))
    assert via.res_d.cpu().numpy().tobytes() == direct.res_d.cpu().numpy().tobytes() and via.res_i.cpu().numpy().tobytes() == direct.res_i.cpu().numpy().tobytes()
    assert not torch.equal(via.planes[1], conv.planes[1])   # (the primitive cell's planes are not the conventional cell's)


def test_the_reward_calculator_on_the_device():
    from matinvent_amd import rewards
    from matinvent_amd.data import SimpleStructure
    calc = rewards.PyMatGen(task="mcia", substrate=[Z.SI_A] * 3 + [90.0] * 3, substrate_millers=[(1, 0, 0)])
    film = lambda a: SimpleStructure([a] * 3, [90.0] * 3, [14], np.zeros((1, 3)))
    out = calc.calc(([film(Z.SI_A), film(float("nan")), film(3.0), film(25.0)], None))
    a2 = float(np.float32(Z.SI_A)) ** 2
    assert abs(out[0] - a2) <= 1e-6 * a2 and np.isnan(out[1]) and abs(out[2] - 117.0) <= 1e-9 and np.isnan(out[3])   # (nothing matches: NaN, as the reference's min([]) raises)
    assert calc.calc([film(3.0)]).tolist() == [out[2]] and calc.bank is not None
