"""Cases of the composition-validity tests (tests/test_chem_host.py, tests/test_gpu_chem.py).

TEST_TABLE is hand-written TEST DATA: seventeen elements with textbook oxidation states and the usual Pauling electronegativities.  It is
not SMACT's table and not a table anybody should filter with.  The synthetic tables serve the edge cases."""
import math

import numpy as np

from tests.chem_ref import SYMBOLS, Z_OF

TEST_TABLE = {
    "H": {"ox": [-1, 1], "eneg": 2.20, "metal": False, "abundance": 1400.0},
    "He": {"ox": [], "eneg": None, "metal": False, "abundance": 0.008},
    "Li": {"ox": [1], "eneg": 0.98, "metal": True, "abundance": 20.0},
    "C": {"ox": [-4, 2, 4], "eneg": 2.55, "metal": False, "abundance": 200.0},
    "N": {"ox": [-3, -2, -1, 1, 2, 3, 4, 5], "eneg": 3.04, "metal": False, "abundance": 19.0},
    "O": {"ox": [-2, -1], "eneg": 3.44, "metal": False, "abundance": 461000.0},
    "F": {"ox": [-1], "eneg": 3.98, "metal": False, "abundance": 585.0},
    "Na": {"ox": [-1, 1], "eneg": 0.93, "metal": True, "abundance": 23600.0},
    "Mg": {"ox": [2], "eneg": 1.31, "metal": True, "abundance": 23300.0},
    "Al": {"ox": [3], "eneg": 1.61, "metal": True, "abundance": 82300.0},
    "Si": {"ox": [-4, 4], "eneg": 1.90, "metal": False, "abundance": 282000.0},
    "S": {"ox": [-2, 2, 4, 6], "eneg": 2.58, "metal": False, "abundance": 350.0},
    "Cl": {"ox": [-1, 1, 3, 5, 7], "eneg": 3.16, "metal": False, "abundance": 145.0},
    "K": {"ox": [1], "eneg": 0.82, "metal": True, "abundance": 20900.0},
    "Ca": {"ox": [2], "eneg": 1.00, "metal": True, "abundance": 41500.0},
    "Fe": {"ox": [2, 3], "eneg": 1.83, "metal": True, "abundance": 56300.0},
    "Cu": {"ox": [1, 2], "eneg": 1.90, "metal": True, "abundance": None},
}


def formula(**counts):
    """formula(Na=1, Cl=1) -> the atomic numbers, in the keyword order."""
    return [Z_OF[s] for s, n in counts.items() for _ in range(n)]


# name -> (types, keywords, expected outputs): the issue's table.  The ALLOY row's first / counts are this build's definition.
NAMED = {
    "NaCl": (formula(Na=1, Cl=1), {}, dict(valid=True, status="ENUMERATED", first=5, n_neutral=2, n_valid=1)),
    "Na2Cl": (formula(Na=2, Cl=1), {}, dict(valid=False, status="ENUMERATED", n_neutral=0)),
    "Fe2O3": (formula(Fe=2, O=3), {}, dict(valid=True, status="ENUMERATED", first=1)),
    "Fe3O4": (formula(Fe=3, O=4), {}, dict(valid=False, status="ENUMERATED")),
    "Li4O2": (formula(Li=4, O=2), {}, dict(valid=True, status="ENUMERATED", counts=[2, 1, 0, 0, 0, 0, 0, 0])),
    "SiC": (formula(Si=1, C=1), {}, dict(valid=True, status="ENUMERATED", first=1, n_neutral=2)),
    "CO2": (formula(C=1, O=2), {}, dict(valid=True, status="ENUMERATED", first=3)),
    "NH3": (formula(N=1, H=3), {}, dict(valid=True, status="ENUMERATED", first=8, n_neutral=2, n_valid=1)),
    "HeO": (formula(He=1, O=1), {}, dict(valid=False, status="NO_STATES")),
    "Si8": (formula(Si=8), {}, dict(valid=True, status="ELEMENTAL")),
    "NaK": (formula(Na=1, K=1), {}, dict(valid=True, status="ALLOY", first=-1, n_neutral=0, n_valid=0, n_combos=0)),
    "NaK_no_alloys": (formula(Na=1, K=1), dict(include_alloys=False), dict(valid=True, status="ENUMERATED", first=0)),
}


def synthetic(radices, zeros=None, eneg=None, metal=False, first_z=1):
    """Elements first_z .. first_z + len(radices) - 1; element e has the states 1 .. radix_e except a 0 at position zeros[e] (None: no
    zero).  With unit counts exactly the combination whose digits are `zeros` is neutral."""
    t = {}
    for e, r in enumerate(radices):
        ox = list(range(1, r + 1))
        if zeros is not None and zeros[e] is not None:
            ox[zeros[e]] = 0
        t[SYMBOLS[first_z + e]] = {"ox": ox, "eneg": (1.0 + 0.1 * e) if eneg is None else eneg[e], "metal": metal}
    return t


def digits(index, radices):
    d = []
    for r in reversed(radices):
        d.append(index % r)
        index //= r
    return d[::-1]


CHUNK_RADICES = ((16, 9, 5, 7, 13), (16, 16, 16, 16), (6, 25, 19, 23))   # N = 65 520, 65 536, 65 550


def chunk_edge_cases():
    """[(name, table, types, index)]: the one neutral combination placed at 0, N - 1, 65 535 and 65 536 where N has that index."""
    out = []
    for radices in CHUNK_RADICES:
        N = math.prod(radices)
        for index in (0, N - 1, 65535, 65536):
            if index < N:
                out.append((f"{'x'.join(map(str, radices))}@{index}", synthetic(radices, digits(index, radices)), list(range(1, len(radices) + 1)), index))
    return out


def dense_table(n_elems, states, first_z=1):
    """Elements with the same signed list each and distinct electronegativities: many neutral combinations, some of them failing the test."""
    return {SYMBOLS[first_z + e]: {"ox": list(states), "eneg": 1.0 + 0.25 * ((e * 5) % n_elems), "metal": False} for e in range(n_elems)}


# The wrap batch: one table of 8 synthetic families on disjoint elements, so that one launch holds crystals of 1 .. 19 chunks.
def wrap_table_and_crystals(n_crystals=300):
    table, kinds = {}, []
    z = 1
    for k in range(1, 20):   # k chunks: N = 63 488 k (k odd) or 65 536 k (k even), the solution at a different place each
        radices = (31 if k % 2 else 32, 32, 32, 2, k)
        N = math.prod(radices)
        index = (N * (k % 7)) // 7 if k % 3 else N - 1
        table.update(synthetic(radices, digits(index, radices), first_z=z))
        kinds.append(list(range(z, z + 5)))
        z += 5
    dense = dense_table(4, range(-8, 8), first_z=z)   # N = 65 536 with thousands of neutral combinations
    table.update(dense)
    kinds.append([z, z, z + 1, z + 2, z + 3, z + 3, z + 3])
    assert z + 4 <= 118
    crystals = [list(kinds[i % len(kinds)]) for i in range(n_crystals)]
    return table, crystals, kinds


def ten_million():
    """Seven lists of ten: N = 10^7 exactly, with signed states so that neutral combinations are plenty.  Elements 1 .. 9 are in the table."""
    return {SYMBOLS[1 + e]: {"ox": list(range(-5, 5)), "eneg": 1.0 + 0.3 * ((e * 4) % 9), "metal": False} for e in range(9)}


def guard_batch():
    """(crystals, expected status names): type 0, type 200, zero atoms, an element absent from TEST_TABLE, between ordinary rows."""
    crystals = [NAMED["NaCl"][0], [11, 0, 17], NAMED["Fe2O3"][0], [200, 8], [], NAMED["NH3"][0], formula(Na=1) + [92], formula(Si=2), [-3], NAMED["CO2"][0]]
    names = ["ENUMERATED", "BAD_INPUT", "ENUMERATED", "BAD_INPUT", "BAD_INPUT", "ENUMERATED", "UNKNOWN_ELEMENT", "ELEMENTAL", "BAD_INPUT", "ENUMERATED"]
    return crystals, names


def shuffled_sizes(seed=5):
    """Crystals of [1, 2, 171, 20, 3] atoms over TEST_TABLE's elements, atom order shuffled."""
    rng = np.random.default_rng(seed)
    out = []
    for n, syms in zip((1, 2, 171, 20, 3), (("Si",), ("Na", "Cl"), ("Fe", "O", "Si"), ("Ca", "C", "O"), ("H", "O"))):
        zs = [Z_OF[s] for s in syms]
        if n == 171:
            types = [zs[0]] * 38 + [zs[1]] * 114 + [zs[2]] * 19   # Fe2 O6 Si1 after the gcd of 19
        elif n == 20:
            types = [zs[0]] * 4 + [zs[1]] * 4 + [zs[2]] * 12      # CaCO3
        elif n == 3:
            types = [zs[0]] * 2 + [zs[1]]
        else:
            types = zs[:n]
        out.append([int(t) for t in rng.permutation(types)])
    return out
