"""The cases of the substrate matcher's tests (tests/test_zsl_host.py, tests/test_gpu_zsl.py): films, banks, parameters and
the restatement of each, computed once, shared and left unchanged."""
from functools import lru_cache

import numpy as np

from tests import zsl_ref64 as R

SI_A = 5.4437   # the conventional cubic cell of silicon


def cubic(a):
    return (np.eye(3) * a).astype(np.float32).reshape(9)


def cell(lengths, angles):
    from matinvent_amd.structure import lattice_matrix
    return lattice_matrix(lengths, angles).astype(np.float32).reshape(9)


def triclinic(seed, n=8):
    """Seeded cells of the size of a 20-atom crystal: edges 4.5 .. 9 A, angles 70 .. 110 degrees."""
    rng = np.random.default_rng(seed)
    return np.stack([cell(rng.uniform(4.5, 9.0, 3), rng.uniform(70.0, 110.0, 3)) for _ in range(n)])


SI_100 = (cubic(SI_A), [(1, 0, 0)])
HEX = (cell([3.19, 3.19, 5.19], [90.0, 90.0, 120.0]), R.planes(1))            # a wurtzite-sized hexagonal substrate, all 13 planes
TETRA = (cell([4.59, 4.59, 2.96], [90.0, 90.0, 90.0]), [(0, 0, 1), (1, 0, 0), (1, 1, 0)])
ORTHO = np.stack([cell([3.9, 5.6, 7.2], [90.0] * 3), cell([4.1, 4.7, 9.3], [90.0] * 3), cell([5.5, 5.5, 10.9], [90.0] * 3)])
# the closed forms on Si (100): edge a (n_f = 1), a / sqrt 2 (2), a / 2 (4), 3.0 (13), and 25 A, whose smallest plane area exceeds max_area
CLOSED = np.stack([cubic(SI_A), cubic(SI_A / np.sqrt(2.0)), cubic(SI_A / 2.0), cubic(3.0), cubic(25.0)])
TRICLINIC_SEED = 52
TRICLINIC = triclinic(TRICLINIC_SEED)
MIXED = np.stack([TRICLINIC[0], TRICLINIC[5], ORTHO[0], cubic(4.05)])
# guards beside a regular film: a NaN lattice, a flat cell, a cell so small that floor(max_area / A) exceeds the cap
NAN_CELL = cubic(4.0).copy()
NAN_CELL[4] = np.nan
FLAT_CELL = np.array([4.0, 0, 0, 0, 5.0, 0, 8.0, 10.0, 0], np.float32)
GUARDS = np.stack([ORTHO[0], NAN_CELL, FLAT_CELL, cubic(1.0), TRICLINIC[1]])

# name: (film cells, film_max_miller, bank, count)
CASES = {
    "closed": (CLOSED, 1, [SI_100], False),
    "closed_count": (CLOSED[[0, 1, 3, 4]], 1, [SI_100], True),   # (a / 2 in count mode decides |1/4 - 4/25| < 0.09: on the tolerance)
    "ortho": (ORTHO, 1, [SI_100, TETRA], False),
    "ortho_count": (ORTHO, 1, [SI_100, TETRA], True),
    "triclinic": (TRICLINIC, 1, [SI_100], False),
    "hex": (MIXED, 1, [HEX], False),
    "bank": (MIXED, 1, [SI_100, HEX, TETRA], False),
    "miller2": (np.stack([TRICLINIC[2], ORTHO[1]]), 2, [SI_100], False),
    "ties": (np.stack([cubic(SI_A)]), 1, [(cubic(SI_A), [(0, 0, 1), (0, 1, 0), (1, 0, 0)])], False),
    "ties_count": (np.stack([cubic(SI_A)]), 1, [(cubic(SI_A), [(0, 0, 1), (0, 1, 0), (1, 0, 0)])], True),
    "guards": (GUARDS, 1, [SI_100], False),
}


@lru_cache(maxsize=None)
def reference(name):
    films, m, bank, count = CASES[name]
    ref = R.analyze(films, R.planes(m), bank, None, count)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


@lru_cache(maxsize=None)
def deviation(name):
    """The restatement's own deviation on a case (tests/zsl_ref64.py deviation): theta and the strains are held to 4 x these."""
    return R.deviation(reference(name))


def widths(bank):
    return sum(len(h) for _, h in bank), len(bank)
