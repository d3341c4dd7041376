"""GPU, end to end: refined_records in the three cells, symmetry_primitive_records and the reward quantities built on them.  A
perturbed crystal loses its group at a hundredth of the tolerance; its refined copy carries all of it there."""
import numpy as np
import pytest

from tests import refine_cases as RC
from tests import refine_ref64 as V
from tests import sm_cases as K
from tests import sym_cases as C
from tests.test_refine_host import record

pytestmark = pytest.mark.gpu


def test_refined_rutile_carries_its_group_at_the_tight_tolerance():
    from matinvent_amd import _lib, symmetry
    rec = record(RC.perturbed()["rutile"])
    amb = record(RC.AMBIGUOUS_CRYSTAL)
    out, res = symmetry.refined_records([rec, amb])
    assert res.status[0] == _lib.SYM_OK and res.n_ops.tolist()[0] == 16 and res.n_orbits.tolist() == [2, 2]
    assert res.status[1] & _lib.SYM_REFINE_FAIL and out[1] is amb and out[0] is not rec   # a failed record comes back as the same object
    assert res.orbits(0).tolist() == [0, 0, 2, 2, 2, 2] and res.multiplicity(0).tolist() == [2, 2, 4, 4, 4, 4] and res.site_symmetry_order(0).tolist() == [8, 8, 4, 4, 4, 4]
    assert res.orbits(1).tolist() == [0, 1] and 0 < res.rms_move[0] <= res.max_move[0] <= 2 * RC.MOVE
    after = symmetry.find_symmetry([out[0]], symprec=RC.SYMPREC_TIGHT)
    before = symmetry.find_symmetry([rec], symprec=RC.SYMPREC_TIGHT)
    assert after.n_ops.tolist() == [16] and after.point_group == ["4/mmm"] and after.status.tolist() == [_lib.SYM_OK]
    assert before.n_ops[0] < 16 and before.point_group != ["4/mmm"]
    # the numbers of the restatement, in A
    ch = V.chain(K.batch([RC.perturbed()["rutile"]]), RC.SYMPREC, K.COS_TOL)
    scale = RC.SYMPREC / ch["tol"][0]
    assert np.isclose(res.max_move[0], ch["ref"]["stat"][0, 0] * scale, rtol=1e-5) and np.isclose(res.cell_change[0], ch["ref"]["stat"][0, 2], rtol=1e-5)


def test_the_primitive_cell_of_refined_rock_salt():
    from matinvent_amd import _lib, symmetry
    rec = record(RC.perturbed()["rocksalt_conv"])
    out, res = symmetry.symmetry_primitive_records([rec])
    assert res.status.tolist() == [_lib.SYM_OK] and len(out[0].species) == 2 and sorted(out[0].species) == [11, 17] and res.n_orbits.tolist() == [2]
    after = symmetry.find_symmetry(out, symprec=RC.SYMPREC_TIGHT)
    assert after.n_ops.tolist() == [48] and after.point_group == ["m-3m"]
    same, _ = symmetry.refined_records([rec], cell="primitive")
    assert np.array_equal(np.asarray(same[0].lengths), np.asarray(out[0].lengths))


def test_the_conventional_cell_of_a_refined_primitive_fcc_cell():
    from matinvent_amd import _lib, symmetry
    fcc = RC.perturb(np.random.default_rng(RC.SEED + 2), K.cell("fcc"))
    out, res = symmetry.refined_records([record(fcc)], cell="conventional")
    assert res.status.tolist() == [_lib.SYM_OK] and len(out[0].species) == 4 and res.n_orbits.tolist() == [1] and res.multiplicity(0).tolist() == [4] * 4
    after = symmetry.find_symmetry(out, symprec=RC.SYMPREC_TIGHT)
    assert after.n_ops.tolist() == [192] and after.point_group == ["m-3m"]
    _, conv = symmetry.conventional_records(out, symprec=RC.SYMPREC_TIGHT)
    assert conv.bravais == ["cF"]
    assert symmetry.find_symmetry([record(fcc)], symprec=RC.SYMPREC_TIGHT).n_ops[0] < 48
    a, b, c, al, be, ga = res.cell_parameters[0]
    assert abs(a / b - 1) < 1e-6 and abs(a / c - 1) < 1e-6 and max(abs(al - 90), abs(be - 90), abs(ga - 90)) < 1e-4


def test_the_reward_quantities():
    from matinvent_amd import rewards
    from matinvent_amd.data import SimpleStructure
    rutile = record(C.known_crystals()["rutile"][0])
    nan_cell = SimpleStructure([4.0, float("nan"), 4.0], [90.0] * 3, [29], np.zeros((1, 3)))
    recs = [rutile, record(RC.AMBIGUOUS_CRYSTAL), record(C.sc_supercell_444()), nan_cell, record(RC.perturbed()["rutile"])]
    out = rewards.Symmetry(quantity="n_orbits").calc((recs, None))
    assert out[0] == 2.0 and np.isnan(out[1:4]).all() and out[4] == 2.0
    d = rewards.Symmetry(quantity="distortion").calc(recs)
    assert d[0] < 1e-6 and np.isnan(d[1:4]).all() and 1e-3 < d[4] <= RC.MOVE
