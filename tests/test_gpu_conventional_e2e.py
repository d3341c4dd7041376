"""GPU, end to end: conventional_records, the reward quantities built on it, and the minimal coincident interface area of a film given in its
primitive cell.  The closed form is DESIGN 52's: a cubic film of the substrate's own lattice constant on Si (1, 0, 0) matches
with n_f = 1 and area a^2."""
import math

import numpy as np
import pytest
import torch

from tests import sm_cases as K
from tests import sym_ref64 as S
from tests import zsl_cases as Z
from tests import zsl_ref64 as ZR
from tests.test_conventional_host import AMBIGUOUS_CRYSTAL, INVARIANCE_BOUND
from tests.test_gpu_zsl import make_bank

pytestmark = pytest.mark.gpu


def record(crystal):
    from matinvent_amd.data import SimpleStructure
    L, z, f = crystal
    L = np.asarray(L, np.float64)
    ln = np.linalg.norm(L, axis=1)
    ang = [math.degrees(math.acos(float(L[i] @ L[j] / (ln[i] * ln[j])))) for i, j in ((1, 2), (0, 2), (0, 1))]
    return SimpleStructure([float(v) for v in ln], ang, list(z), np.asarray(f, np.float64))


def fcc_primitive(a, z=14):
    from matinvent_amd.data import SimpleStructure
    return SimpleStructure([a / math.sqrt(2.0)] * 3, [60.0] * 3, [z], np.zeros((1, 3)))


def test_conventional_records_on_primitive_rock_salt():
    from matinvent_amd import _lib, symmetry
    tri = record(K.random_crystal(np.random.default_rng(3), [2, 1]))
    amb = record(AMBIGUOUS_CRYSTAL)
    out, res = symmetry.conventional_records([record(K.cell("rocksalt_prim")), amb, tri])
    assert len(out) == 3 and res.bravais == ["cF", "", "aP"] and res.centring == ["F", "", "P"] and res.mult.tolist() == [4, 1, 1]
    assert res.status[0] == _lib.SYM_OK and res.status[1] & _lib.SYM_CONV_FAIL and out[1] is amb   # a failed record comes back as it was
    assert sorted(out[0].species) == [11] * 4 + [17] * 4 and abs(round(abs(np.linalg.det(res.M[0])))) == 4
    p = res.cell_parameters[0]
    assert np.abs(p[:3] / K.A0 - 1.0).max() <= INVARIANCE_BOUND and np.abs(p[3:] / 90.0 - 1.0).max() <= INVARIANCE_BOUND, p
    assert np.allclose(out[0].lengths, p[:3]) and np.allclose(out[0].angles, p[3:]) and len(out[2].species) == 3
    f = np.asarray(out[0].frac_coords if hasattr(out[0], "frac_coords") else out[0].coords, np.float64)
    assert np.abs(2 * f - np.round(2 * f)).max() < 1e-6   # every atom on the half-integer grid of the cube


def test_the_reward_quantities():
    from matinvent_amd import rewards
    tri = record(K.random_crystal(np.random.default_rng(3), [2, 1]))
    recs = [record(K.cell("fcc")), tri, record(AMBIGUOUS_CRYSTAL), record(K.cell("bcc"))]
    out = rewards.Symmetry(quantity="bravais").calc((recs, None))
    assert out[0] == 14.0 and out[1] == 1.0 and np.isnan(out[2]) and out[3] == 13.0
    mult = rewards.Symmetry(quantity="centring_mult").calc(recs)
    assert mult[0] == 4.0 and mult[1] == 1.0 and np.isnan(mult[2]) and mult[3] == 2.0


def test_mcia_of_a_primitive_fcc_film_in_its_conventional_cell():
    from matinvent_amd import rewards, substrates
    from matinvent_amd.data import SimpleStructure
    zsl = substrates.ZSL()
    bank = make_bank([Z.SI_100], zsl, fill=None)
    a = Z.SI_A
    prim, cube = fcc_primitive(a), SimpleStructure([a] * 3, [90.0] * 3, [14] * 4, np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]], float))
    conv = substrates.match_records(zsl, [prim], bank, conventional=True)
    direct = substrates.match_records(zsl, [cube], bank)
    as_given = substrates.match_records(zsl, [prim], bank)
    print("mcia of the primitive fcc film: conventional=True %.6f, the cube given directly %.6f, conventional=False %.6f (recorded)"
          % (conv.mcia[0, 0], direct.mcia[0, 0], as_given.mcia[0, 0]))
    a2 = float(np.float32(a)) ** 2
    assert conv.mcia_status[0, 0] == ZR.OK and conv.n_f[0, 0] == 1 and abs(conv.mcia[0, 0] - a2) <= 1e-6 * a2 and abs(conv.area[0, 0] - a2) <= 1e-6 * a2
    assert torch.equal(conv.res_i, direct.res_i) and torch.equal(conv.res_n, direct.res_n) and torch.equal(conv.d_mcia_plane, direct.d_mcia_plane)
    area, status = substrates.mcia([prim], bank, zsl, conventional=True)
    assert status[0] == ZR.OK and area[0] == conv.mcia[0, 0]
    calc = rewards.PyMatGen(task="mcia", substrate=[a] * 3 + [90.0] * 3, substrate_millers=[(1, 0, 0)], conventional=True)
    assert calc.calc(([prim], None)).tolist() == [conv.mcia[0, 0]]
    with pytest.raises(ValueError, match="exclude each other"):
        substrates.match_records(zsl, [prim], bank, primitive=True, conventional=True)
    # a substrate given as a record with atoms is put into its conventional cell like the films
    sub_area, sub_status = substrates.mcia([cube], prim, zsl, conventional=True)
    assert sub_status[0] == ZR.OK and abs(sub_area[0] - a2) <= 1e-6 * a2


def test_without_the_keyword_match_records_is_the_parent():
    """The films of the substrate matcher's own record test, conventional unset: every array equals the restatement's reference as it did
    before the keyword, and equals the arrays of the records' cells matched directly."""
    from matinvent_amd import substrates
    from matinvent_amd.data import SimpleStructure
    zsl = substrates.ZSL()
    bank = make_bank([Z.SI_100, Z.TETRA], zsl, fill=None)
    recs = [SimpleStructure([3.9, 5.6, 7.2], [90.0] * 3, [8], np.zeros((1, 3))), "not a crystal", SimpleStructure([4.1, 4.7, 9.3], [90.0] * 3, [8], np.zeros((1, 3)))]
    res = substrates.match_records(zsl, recs, bank)
    ref = Z.reference("ortho")
    for k, b in ((0, 0), (2, 1)):
        assert np.array_equal(res.area[k], ref["res_d"][b, :, 0]) and np.array_equal(res.n_f[k], ref["res_i"][b, :, 2]) and np.array_equal(res.mcia[k], ref["mcia"][b])
        assert np.array_equal(res.film_hnf[k], ref["res_i"][b, :, 4:7]) and np.array_equal(res.sub_hnf[k], ref["res_i"][b, :, 7:10])
    plain = substrates.match_arrays(zsl, torch.from_numpy(substrates.record_cells(recs)).to(bank.device), bank)
    off = substrates.match_records(zsl, recs, bank, conventional=False)
    for other in (plain, off):
        for k in ("res_d", "res_i", "res_n", "d_mcia", "d_mcia_plane", "d_mcia_status"):
            a, b = getattr(res, k), getattr(other, k)   # (the bits: rows without a match hold NaN)
            assert a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), k
