"""Inputs shared by the symmetry constraint's CPU and GPU tests: the crystals of tests/refine_cases.py with the operations the
exact restatement chain finds for them, carried into each crystal's own basis, a hand-built 171-atom P-1 crystal, and the constraints built
from them once."""
from functools import lru_cache

import numpy as np

from tests import refine_cases as RC
from tests import refine_ref64 as V
from tests import sm_cases as K

NAMES = ("one_atom_cubic", "p1bar_pair", "rutile", "wurtzite", "rocksalt_conv", "pm3m_64", "p1bar_171")


def p1bar_pair():
    rng = np.random.default_rng(56)
    x = rng.uniform(0.05, 0.45, (1, 3))
    return K.triclinic(rng), [14, 14], np.concatenate([x, 1.0 - x])


def p1bar_171():
    """One atom on the centre of inversion and 85 pairs (x, -x): more atoms than the finder takes, so its two operations are written down."""
    rng = np.random.default_rng(171)
    x = rng.uniform(0.02, 0.48, (85, 3))
    return K.triclinic(rng, 3.0), [26] + [8] * 170, np.concatenate([np.zeros((1, 3)), x, 1.0 - x])


def crystal(name):
    if name == "one_atom_cubic":
        return RC.one_atom_cubic()
    if name == "p1bar_pair":
        return p1bar_pair()
    if name == "p1bar_171":
        return p1bar_171()
    return RC.base(name)


@lru_cache(maxsize=None)
def operations(name):
    """(W [K, 3, 3] int, t [K, 3]) of the crystal in its own basis: g_k(f) = f W_k^-1 + t_k."""
    if name == "p1bar_171":
        return np.stack([np.eye(3, dtype=np.int64), -np.eye(3, dtype=np.int64)]), np.zeros((2, 3))
    ch = V.chain_exact([crystal(name)], RC.SYMPREC_TIGHT, K.COS_TOL)
    ex = ch["ref"]["extra"][0]
    assert ex is not None and int(ch["ref"]["info"][0][7]) == 0
    T = np.array(ex["T"], np.int64).reshape(3, 3)              # reduced cell = T x cell, f = f_r T
    Ti = np.round(np.linalg.inv(T.astype(np.float64))).astype(np.int64)
    W = np.stack([Ti @ np.asarray(Wr, np.int64).reshape(3, 3) @ T for Wr in ex["rot"]])
    return W, np.asarray(ex["tbar"], np.float64) @ T.astype(np.float64)


@lru_cache(maxsize=None)
def constraint(name):
    from matinvent_amd.symmetry_constraint import SymmetryConstraint
    L, z, f = crystal(name)
    W, t = operations(name)
    return SymmetryConstraint.from_operations(len(z), f, W, t, tol=1e-6, atom_types=z)


EXPECTED_OPS = {"one_atom_cubic": 48, "p1bar_pair": 2, "rutile": 16, "wurtzite": 12, "rocksalt_conv": 192, "pm3m_64": 48, "p1bar_171": 2}


def guard_case():
    """(constraint, atom_types, frac, lat): rutile, rutile with a NaN cell, rutile with a flat cell (its c row is zero: the last pivot is 0),
    a free crystal, rock salt.  The two failed cells keep every bit and count one failure each."""
    from matinvent_amd import symmetry_constraint as SC
    from tests import symc_ref64 as V
    c = SC.stack([constraint("rutile")] * 3 + [SC.SymmetryConstraint.identity([5]), constraint("rocksalt_conv")])
    a, x, l = V.random_state(np.random.default_rng(99), [int(v) for v in c.num_atoms])
    l[1, 4] = np.float32("nan")
    l[2] = np.array([4, 0, 0, 0, 4, 0, 0, 0, 0], np.float32)
    return c, a, x, l


GUARD_FAILURES = [0, 1, 1, 0, 0]


def batch_300():
    """300 crystals of 1 .. 3 atoms -- the one-atom cube under its 48 operations, the P-1 pair, a free crystal of three atoms -- with rock
    salt at positions 0, 150 and 299."""
    from matinvent_amd import symmetry_constraint as SC
    small = [constraint("one_atom_cubic"), constraint("p1bar_pair"), SC.SymmetryConstraint.identity([3])]
    parts = [small[i % 3] for i in range(300)]
    for pos in (0, 150, 299):
        parts[pos] = constraint("rocksalt_conv")
    return SC.stack(parts)
