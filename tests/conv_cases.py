"""Inputs shared by the conventional cell's CPU and GPU tests: the 14 Bravais lattices as one-atom primitive cells, the known
crystals of tests/sym_cases.py, crystals of lower symmetry in a metric of higher symmetry, each beside a transformed copy, and the
restatement's chain over all of them computed once.  An expectation is (crystal system 1 .. 7, mult, centring letter or None for "any")."""
import math
from functools import lru_cache

import numpy as np

from tests import conv_ref64 as V
from tests import sm_cases as K
from tests import sym_cases as C

SYMPREC, ANGLE_TOL = 0.1, 5.0
A, B_LEN, C_LEN = 3.1, 4.3, 5.9


def one(L):
    return np.asarray(L, np.float64), [29], np.zeros((1, 3))


def lattices():
    """name -> (crystal, expectation): the 14 Bravais lattices, 17 settings."""
    a, b, c = A, B_LEN, C_LEN
    r3 = math.sqrt(3) / 2
    rng = np.random.default_rng(5)
    return {
        "cP": (one(np.eye(3) * a), (7, 1, "P")), "cI": (one(K.BCC), (7, 2, "I")), "cF": (one(K.FCC), (7, 4, "F")),
        "tP": (one(np.diag([a, a, c])), (4, 1, "P")),
        "tI_tall": (one([[a, 0, 0], [0, a, 0], [a / 2, a / 2, c / 2]]), (4, 2, "I")),
        "tI_flat": (one([[c, 0, 0], [0, c, 0], [c / 2, c / 2, a / 2]]), (4, 2, "I")),
        "oP": (one(np.diag([a, b, c])), (3, 1, "P")),
        "oI": (one([[a, 0, 0], [0, b, 0], [a / 2, b / 2, c / 2]]), (3, 2, "I")),
        "oF": (one([[0, b / 2, c / 2], [a / 2, 0, c / 2], [a / 2, b / 2, 0]]), (3, 4, "F")),
        "oS_C": (one([[a / 2, b / 2, 0], [-a / 2, b / 2, 0], [0, 0, c]]), (3, 2, "C")),
        "oS_A": (one([[a, 0, 0], [0, b / 2, c / 2], [0, -b / 2, c / 2]]), (3, 2, "C")),
        "hP": (one(K.HEX), (6, 1, "P")),
        "hR_tall": (one([[2.9, 0, 1.7], [-1.45, 2.9 * r3, 1.7], [-1.45, -2.9 * r3, 1.7]]), (5, 3, "R")),
        "hR_flat": (one([[2.9, 0, 0.6], [-1.45, 2.9 * r3, 0.6], [-1.45, -2.9 * r3, 0.6]]), (5, 3, "R")),
        "mP": (one([[a, 0, 0], [0, b, 0], [c * math.cos(1.9), 0, c * math.sin(1.9)]]), (2, 1, "P")),
        "mS": (one([[a / 2, b / 2, 0], [-a / 2, b / 2, 0], [c * math.cos(1.9), 0, c * math.sin(1.9)]]), (2, 2, None)),
        "aP": ((K.triclinic(rng, 1.0), [29], np.zeros((1, 3))), (1, 1, "P")),
    }


def pyrite(u=0.385):
    s8 = [(u, u, u), (-u, -u, -u), (.5 + u, .5 - u, -u), (.5 - u, .5 + u, u), (-u, .5 + u, .5 - u), (u, .5 - u, .5 + u), (.5 - u, -u, .5 + u), (.5 + u, u, .5 - u)]
    f = [[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]] + [[x % 1.0 for x in s] for s in s8]
    return np.eye(3) * 5.4, [26] * 4 + [16] * 8, np.array(f, np.float64)


def lower_symmetry():
    """Crystals whose atoms lower the symmetry of their metric."""
    cube = np.eye(3) * 4.0
    return {
        "cubic_metric_4mm": ((cube, [11, 17], np.array([[0, 0, 0], [0, 0, .3]])), (4, 1, "P")),
        "cubic_metric_mm2": ((cube, [11, 17, 17], np.array([[0, 0, 0], [.2, 0, .3], [.8, 0, .3]])), (3, 1, "P")),
        "cubic_metric_m": ((cube, [11, 17, 17], np.array([[0, 0, 0], [.13, 0, .3], [.37, 0, .21]])), (2, 1, "P")),
        "hex_metric_3m": ((K.HEX, [11, 17], np.array([[0, 0, 0], [1 / 3, 2 / 3, .3]])), (5, 1, "P")),
        "fcc_metric_tI": ((K.FCC, [11, 17], np.array([[0, 0, 0], [.3, .3, -.3]]) % 1.0), (4, 2, "I")),
        "pyrite": (pyrite(), (7, 1, "P")),
    }


KNOWN_EXPECT = {"sc": (7, 1, "P"), "fcc": (7, 4, "F"), "bcc": (7, 2, "I"), "diamond": (7, 4, "F"), "zincblende": (7, 4, "F"), "rocksalt_conv": (7, 4, "F"),
                "cscl": (7, 1, "P"), "hcp": (6, 1, "P"), "wurtzite": (6, 1, "P"), "rutile": (4, 1, "P"), "triclinic": (1, 1, "P"),
                "triclinic_inversion": (1, 1, "P"), "triclinic_2x1x1": (1, 1, "P")}


@lru_cache(maxsize=None)
def all_cases():
    """[(name, crystal, expectation)]: every lattice and every lower-symmetry crystal as typed and as a transformed copy ("name~"), then the
    known crystals."""
    rng = np.random.default_rng(71)
    out = []
    for group in (lattices(), lower_symmetry()):
        for name, (crystal, expect) in group.items():
            crystal = (np.asarray(crystal[0], np.float64), list(crystal[1]), np.asarray(crystal[2], np.float64))
            out.append((name, crystal, expect))
            out.append((name + "~", K.transformed(rng, crystal), expect))
    for name, v in C.known_crystals().items():
        out.append((name, v[0], KNOWN_EXPECT[name]))
    return out


@lru_cache(maxsize=None)
def fixture_results():
    """(cases, batch, chain) of all_cases() under the restatement, unwritten rows 0."""
    cases = all_cases()
    batch = K.batch([c[1] for c in cases])
    return cases, batch, V.chain(batch, SYMPREC, K.COS_TOL)


@lru_cache(maxsize=None)
def random_results():
    crystals = C.random_set()
    batch = K.batch(crystals)
    return crystals, batch, V.chain(batch, SYMPREC, K.COS_TOL)


def rocksalt_prim():
    return K.cell("rocksalt_prim")
