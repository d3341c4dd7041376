"""GPU: the structure matcher's host API (matinvent_amd/matching.py) on a small set with planted duplicates -- transformed and
slightly displaced copies: rms_dist, fit, novel_mask, unique_mask and the StructureBank round trip."""
import numpy as np
import pytest
import torch

from tests import sm_cases as K

pytestmark = pytest.mark.gpu


def record(crystal):
    from matinvent_amd.data import SimpleStructure
    L, z, f = crystal
    L = np.asarray(L, np.float64)
    lengths = np.linalg.norm(L, axis=1)
    cos = lambda u, v: float(np.dot(u, v) / (np.linalg.norm(u) * np.linalg.norm(v)))
    angles = [float(np.degrees(np.arccos(c))) for c in (cos(L[1], L[2]), cos(L[0], L[2]), cos(L[0], L[1]))]
    return SimpleStructure(lengths.tolist(), angles, [int(v) for v in z], np.asarray(f, np.float64))


@pytest.fixture(scope="module")
def planted():
    """Records 0 .. 3 distinct (two of one formula and atom count), 4 a copy of 0, 5 a copy of 2, 6 a copy of 0 again."""
    rng = np.random.default_rng(21)
    a, b = K.random_crystal(rng, [4, 2, 2]), K.random_crystal(rng, [4, 2, 2])
    c, d = K.random_crystal(rng, [3, 3]), K.cell("rocksalt_conv")
    crystals = [a, b, c, d, K.transformed(rng, a, sigma=0.004), K.transformed(rng, c, sigma=0.004), K.transformed(rng, a, sigma=0.004)]
    return [record(x) for x in crystals]


def test_rms_dist_and_fit(planted):
    from matinvent_amd import matching
    d = matching.rms_dist(planted[0], planted[4])
    assert d is not None and 0 < d[0] < 0.05 and d[0] <= d[1]
    assert matching.fit(planted[0], planted[4]) and matching.fit(planted[2], planted[5])
    assert not matching.fit(planted[0], planted[1])          # one formula, another structure
    assert matching.rms_dist(planted[0], planted[2]) is None and not matching.fit(planted[0], planted[3])   # other compositions


def test_unique_mask_keeps_the_planted_uniques_in_list_order(planted):
    from matinvent_amd import matching
    assert matching.unique_mask(planted).tolist() == [True, True, True, True, False, False, False]
    # reversed: copy of 0, copy of 2, copy of 0 (repeat), 3, 2 (repeat of its copy), 1, 0 (repeat)
    assert matching.unique_mask(planted[::-1]).tolist() == [True, True, False, True, False, True, False]
    assert matching.unique_mask([]).shape == (0,)


def test_novel_mask_and_the_bank_round_trip(planted, tmp_path):
    from matinvent_amd import matching
    bank = matching.StructureBank.from_records(planted[:2])
    novel, rms = matching.novel_mask(planted, bank, return_rms=True)
    assert novel.tolist() == [False, False, True, True, False, True, False]
    assert rms[0] < 1e-6 and rms[4] < 0.05 and np.isinf(rms[2])
    path = bank.save(str(tmp_path / "bank.npz"))
    again = matching.StructureBank.load(path)
    assert len(again) == 2 and again.keys == bank.keys
    for k in ("lat", "inv", "frac", "types", "perm", "spec_Z", "spec_off", "info"):
        assert torch.equal(getattr(again.prepared, k), getattr(bank.prepared, k)), k
    novel2, rms2 = matching.novel_mask(planted, again, return_rms=True)
    assert np.array_equal(novel, novel2) and np.array_equal(rms, rms2)
    bank.add([planted[2]])                                   # an append: a second call's repeat is no longer novel
    assert matching.novel_mask(planted, bank).tolist() == [False, False, False, True, False, False, False]


def test_a_flagged_record_matches_by_formula_alone(planted):
    from matinvent_amd import matching
    from matinvent_amd.data import SimpleStructure
    bad = SimpleStructure(planted[0].lengths, planted[0].angles, planted[0].species, np.full_like(planted[0].frac_coords, np.nan))
    other = SimpleStructure([3.0, 3.0, 3.0], [90.0, 90.0, 90.0], [5], np.full((1, 3), np.nan))
    bank = matching.StructureBank.from_records(planted[:1])
    assert matching.novel_mask([bad, other], bank).tolist() == [False, True]
    assert matching.unique_mask([bad, bad, planted[0], other]).tolist() == [True, False, True, True]


def test_unfilter_structure_mode_keeps_the_planted_uniques_and_remembers(planted):
    from matinvent_amd.novelty import UNFilter
    flt = UNFilter(matcher="structure", remember=True)
    data = list(range(len(planted)))
    kept_data, kept, m = flt(data, planted)
    assert kept_data == [0, 1, 2, 3] and kept == planted[:4]
    assert m["unique_frac"] == 4 / 7 and m["novel_frac"] == 1.0 and m["bank_size"] == 4.0 and np.isnan(m["match_rms_mean"])
    kept_data, kept, m = flt(data, planted)                  # the second call: every record repeats a remembered one
    assert kept_data == [] and m["novel_frac"] == 0.0 and m["bank_size"] == 4.0 and 0 <= m["match_rms_mean"] < 0.05
    with pytest.raises(ValueError, match="matcher"):
        UNFilter(matcher="pymatgen")


def test_sunfilter_passes_the_matcher_through(planted, tmp_path):
    from matinvent_amd import matching
    from matinvent_amd.stability import SUNFilter
    path = matching.StructureBank.from_records(planted[1:2]).save(str(tmp_path / "ref.npz"))
    flt = SUNFilter(metrics=["unique", "novel"], matcher="structure", reference_path=path, stol=0.3, ltol=0.2, angle_tol=5.0)
    assert flt.un.matcher == "structure" and isinstance(flt.un.bank, matching.StructureBank)
    data, kept, m = flt(list(range(len(planted))), planted)
    assert data == [0, 2, 3] and m["match_rms_mean"] < 1e-6 and m["bank_size"] == 1.0


def test_fingerprint_mode_is_the_default_and_unchanged(planted):
    """The default UNFilter takes the parent's path: a FingerprintBank, no structure-matcher key in the metrics, and the masks of
    novelty.unique_mask / novel_mask on the same records."""
    from matinvent_amd import novelty
    flt = novelty.UNFilter()
    assert flt.matcher == "fingerprint" and isinstance(flt.bank, novelty.FingerprintBank)
    data, kept, m = flt(list(range(len(planted))), planted)
    assert "match_rms_mean" not in m
    want = novelty.unique_mask(planted) & novelty.novel_mask(planted, novelty.FingerprintBank())
    assert data == [i for i in range(len(planted)) if want[i]]


def test_build_structure_bank_script(planted, tmp_path):
    import subprocess
    import sys
    from matinvent_amd import matching
    from matinvent_amd.structure import write_extxyz
    from tests.header_util import ROOT
    src, dst = write_extxyz(planted[:3], str(tmp_path / "in.extxyz")), str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, f"{ROOT}/scripts/build_structure_bank.py", src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    bank = matching.StructureBank.load(dst)
    assert len(bank) == 3 and matching.novel_mask(planted, bank).tolist() == [False, False, False, True, False, False, False]
