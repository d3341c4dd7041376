"""GPU: the symmetry finder's host API (matinvent_amd/symmetry.py) and the structure matcher on primitive cells: a
conventional and a primitive cell of one structure match with primitive=True and only then, the default leaves every prepared bit as it
was, and rewards.Symmetry reads the counts."""
import numpy as np
import pytest
import torch

from tests import sm_cases as K
from tests import sm_ref64 as R
from tests.test_gpu_struct_match_e2e import record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cells():
    rng = np.random.default_rng(71)
    zb = (K.FCC, [30, 16], np.array([[0, 0, 0], [.25, .25, .25]]))
    return {"conv": record(K.cell("rocksalt_conv")), "prim": record(K.cell("rocksalt_prim")), "zincblende": record(zb),
            "triclinic": record(K.random_crystal(rng, [2, 1]))}


def test_conventional_and_primitive_rock_salt_match_on_primitive_cells_only(cells):
    from matinvent_amd import matching
    assert matching.fit(cells["conv"], cells["prim"], primitive=True)
    d = matching.rms_dist(cells["conv"], cells["prim"], primitive=True)
    assert d is not None and d[0] < 1e-5
    assert matching.rms_dist(cells["conv"], cells["prim"]) is None and not matching.fit(cells["conv"], cells["prim"])
    assert not matching.fit(cells["conv"], cells["zincblende"], primitive=True)


def test_unique_and_novel_masks_on_primitive_cells(cells):
    from matinvent_amd import matching
    from matinvent_amd.novelty import UNFilter
    trio = [cells["conv"], cells["prim"], cells["zincblende"]]
    assert matching.unique_mask(trio, primitive=True).tolist() == [True, False, True]
    assert matching.unique_mask(trio).tolist() == [True, True, True]
    bank = matching.StructureBank.from_records([cells["conv"]], primitive=True)
    assert [k[1] for k in bank.keys] == [2] and bank.na[0].tolist() == [2]   # the index keys on the primitive atom count
    assert matching.novel_mask(trio, bank).tolist() == [False, False, True]
    plain = matching.StructureBank.from_records([cells["conv"]])
    assert [k[1] for k in plain.keys] == [8] and matching.novel_mask(trio, plain).tolist() == [False, True, True]
    flt = UNFilter(matcher="structure", primitive=True)
    _, kept, m = flt(None, trio)
    assert len(kept) == 2 and m["unique_frac"] == pytest.approx(2 / 3)


def test_the_default_prepares_every_bit_as_before(cells):
    """primitive=False on regular_set(): equal to the restatement the parent's kernel is held to, and to the set prepared from the arrays."""
    from matinvent_amd import matching
    from matinvent_amd.structure import record_arrays
    crystals, _ = K.regular_set()
    records = [record(c) for c in crystals]
    na, types, frac, lat = record_arrays(records)
    off = np.concatenate([[0], np.cumsum(na.numpy())]).astype(np.int32)
    P = R.prepare(off, types.numpy(), frac.numpy(), lat.reshape(-1, 9).numpy())
    S = matching.prepare(records)
    again = matching.prepare(records, primitive=False)
    for k in ("lat", "inv", "frac", "types", "perm", "spec_Z", "spec_off", "info"):
        assert np.array_equal(getattr(S, k).cpu().numpy()[:len(P[k])], P[k]), k
        assert torch.equal(getattr(S, k), getattr(again, k)), k


def test_find_symmetry_and_primitive_records(cells):
    from matinvent_amd import _lib, symmetry
    recs = [cells["conv"], cells["prim"], cells["zincblende"], cells["triclinic"]]
    res = symmetry.find_symmetry(recs)
    assert res.n_ops.tolist() == [192, 48, 24, 1] and res.n_trans.tolist() == [4, 1, 1, 1] and (res.status == _lib.SYM_OK).all()
    assert res.point_group == ["m-3m", "m-3m", "-43m", "1"] and res.crystal_system_name == ["cubic", "cubic", "cubic", "triclinic"]
    W, t, dev = res.operations(2)
    assert W.shape == (24, 3, 3) and t.shape == (24, 3) and (np.abs(np.linalg.det(W.astype(np.float64))).round() == 1).all() and dev.max() < 1e-6
    prim, n_trans = symmetry.primitive_records(recs)
    assert [len(p.species) for p in prim] == [2, 2, 2, 3] and n_trans.tolist() == [4, 1, 1, 1]
    assert sorted(prim[0].species) == [11, 17] and np.allclose(prim[0].lengths, [K.A0 / np.sqrt(2)] * 3, atol=1e-5)
    assert np.array_equal(np.asarray(prim[3].frac_coords, np.float32), np.asarray(recs[3].frac_coords, np.float32))


def test_symmetry_reward(cells, tmp_path):
    from matinvent_amd import rewards
    recs = [cells["conv"], cells["triclinic"]]
    got = {q: rewards.Symmetry(quantity=q).calc(recs).tolist() for q in ("n_ops", "pg_order", "not_p1", "crystal_system")}
    assert got == {"n_ops": [192.0, 1.0], "pg_order": [48.0, 1.0], "not_p1": [1.0, 0.0], "crystal_system": [7.0, 1.0]}
    big = record(K.random_crystal(np.random.default_rng(5), [65]))
    assert np.isnan(rewards.Symmetry().calc([big, cells["prim"]])).tolist() == [True, False]
    rw = rewards.Reward(str(tmp_path / "rewards"), [dict(name="symmetry", calculator=rewards.Symmetry("pg_order"), target="ascending", minv=1.0, maxv=48.0)], 0.5)
    r, props, failed = rw.scoring(recs + [big])
    assert r.tolist() == [1.0, 0.0, 0.0] and failed.tolist() == [False, False, True]
    with pytest.raises(ValueError):
        rewards.Symmetry(quantity="hall_number")
