"""CPU checks of the fingerprint layer that needs no GPU: tests/fp_ref64.py (the float64 restatement the GPU tests compare the kernel
with) against a brute-force element-by-element evaluation on tiny cells; its invariance under the re-descriptions of one crystal at the
float64 rounding level; two structures of one formula well apart; the new header's symbols and the ctypes table."""
import numpy as np
import pytest

from matinvent_amd import _lib
from tests import fp_ref64 as R
from tests.header_util import declared_symbols

SEPARATION = 0.05   # d(rock salt, CsCl type) must exceed this: a hundred times the rattle distances of DESIGN 32, a tenth of what is measured


@pytest.mark.parametrize("case", ["one", "two_species", "skew"])
def test_restatement_is_the_definition_element_by_element(case):
    r_max, nbins, sigma = 3.0, 6, 0.2
    c = {"one": (np.array([26]), np.array([[0.3, 0.1, 0.8]]), np.eye(3) * 2.2),
         "two_species": (np.array([8, 3, 8]), np.array([[0.1, 0.2, 0.3], [0.5, 0.6, 0.1], [0.8, 0.3, 0.7]]), np.diag([2.5, 3.0, 2.8])),
         "skew": (np.array([3, 8]), np.array([[0.0, 0.0, 0.0], [0.4, 0.5, 0.6]]), np.array([[2.6, 0, 0], [1.5, 2.4, 0], [0.4, 0.3, 2.9]]))}[case]
    ref = R.fingerprint(*c, r_max=r_max, nbins=nbins, sigma=sigma)
    want = R.brute(*c, r_max, nbins, sigma, reach=4)        # |T| <= 4 cells of >= 2.2 A covers r_max + 12 sigma = 5.4 A
    assert ref["status"] == R.OK and abs(np.linalg.norm(ref["u"]) - 1) < 1e-14
    assert np.abs(ref["u"] - want).max() < 1e-13
    f32 = R.fingerprint(*c, r_max=r_max, nbins=nbins, sigma=sigma, dtype=np.float32)
    assert f32["u"].dtype == np.float32 and 0 < np.abs(f32["u"] - ref["u"]).max() < 1e-5


@pytest.mark.parametrize("name", ["five_atoms", "skewed", "eight_species"])
def test_redescriptions_are_invisible_at_float64_rounding(name):
    c = R.kernel_cases()[name]
    u = R.fingerprint(*c)["u"]
    for what, f in R.REDESCRIPTIONS:
        d = R.distance(u, R.fingerprint(*f(c))["u"])
        assert abs(d) < 1e-13, (what, d)


def test_two_structures_of_one_formula_are_well_separated():
    d = R.distance(R.fingerprint(*R.rock_salt())["u"], R.fingerprint(*R.cscl_type())["u"])
    print(f"d(rock salt, CsCl type) = {d:.4f}")
    assert d > SEPARATION
    t, x, L = R.rock_salt()
    g = np.random.default_rng(0)
    rattled = (t, x + g.normal(0, 0.05, x.shape) @ np.linalg.inv(L), L)
    assert R.distance(R.fingerprint(t, x, L)["u"], R.fingerprint(*rattled)["u"]) < SEPARATION / 10


def test_verdicts_and_flagged_rows():
    for name, (t, x, L, status) in R.flagged_cases().items():
        ref = R.fingerprint(t, x, L)
        assert ref["status"] == status and not ref["u"].any(), name
    nine = R.fingerprint(*R.kernel_cases()["nine_species"])
    assert nine["status"] == R.SPECIES and nine["m"] == 9 and not nine["u"].any()
    assert R.verdict(np.array([0, 3]), np.zeros((2, 3)), np.eye(3) * 4)[0] == R.ATOMS
    assert R.verdict(np.zeros(0), np.zeros((0, 3)), np.eye(3) * 4)[0] == R.ATOMS
    # the reach comes from the perpendicular heights: the skewed cell's edge b is 6.0 A, its height along b 2.4 A
    st, m, images, _ = R.verdict(*R.kernel_cases()["skewed"])
    by_lengths = np.prod(2 * np.ceil((R.R_MAX + R.CUT * R.SIGMA) / np.linalg.norm(R.SKEWED, axis=1) + 0.5) + 1)
    assert st == R.OK and images > by_lengths


def test_header_symbols_and_table():
    names = declared_symbols("matinvent_hip_fp.h")
    assert names == ["mi_structure_fingerprint", "mi_structure_fingerprint_offsets"] and sorted(_lib.FP_SIGNATURES) == names
    assert any(t is _lib.FP_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    assert [f for f, _ in _lib.FpParams._fields_] == ["r_max", "sigma", "nbins"]
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "matinvent_hip_fp.h")).read()
    macro = lambda k: float(re.search(rf"#define {k}\s+([0-9.]+)", src).group(1))
    assert (macro("MI_FP_MAX_SPECIES"), macro("MI_FP_MAX_BLOCKS"), macro("MI_FP_MAX_BINS"), macro("MI_FP_MAX_REACH"), macro("MI_FP_CUT")) == \
        (_lib.FP_MAX_SPECIES, _lib.FP_MAX_BLOCKS, _lib.FP_MAX_BINS, _lib.FP_MAX_REACH, _lib.FP_CUT) == (R.MAX_SPECIES, R.MAX_BLOCKS, R.MAX_BINS, R.MAX_REACH, R.CUT)
    assert macro("MI_FP_MIN_VOLUME") == R.MIN_VOLUME and R.CUT >= 5
    assert [macro(f"MI_FP_{k}") for k in ("OK", "SPECIES", "NONFINITE", "VOLUME", "REACH", "ATOMS")] == \
        [_lib.FP_OK, _lib.FP_SPECIES, _lib.FP_NONFINITE, _lib.FP_VOLUME, _lib.FP_REACH, _lib.FP_ATOMS] == [R.OK, R.SPECIES, R.NONFINITE, R.VOLUME, R.REACH, R.ATOMS]
