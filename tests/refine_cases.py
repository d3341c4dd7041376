"""Inputs shared by the refined structure's CPU and GPU tests: the known crystals of tests/sym_cases.py with their orbits, a
constructed 64-atom Pm-3m cell, perturbed copies (atoms moved by at most 0.02 A, a symmetric strain of at most 0.002 an entry), a transformed
copy of each perturbed crystal, the guard batch, and the restatement's results computed once."""
import itertools
from functools import lru_cache

import numpy as np

from tests import refine_ref64 as V
from tests import sm_cases as K
from tests import sym_cases as C

SYMPREC, SYMPREC_TIGHT = 0.1, 1e-3
MOVE, STRAIN = 0.02, 0.002
SEED = 55
PERTURBED = ("rutile", "wurtzite", "rocksalt_conv", "hcp", "pm3m_64")
# name -> [(atoms of the orbit, site order)] per orbit, in the order of the crystal's atoms
KNOWN_ORBITS = {
    "rutile": [(2, 8), (4, 4)],
    "rocksalt_conv": [(4, 48), (4, 48)],
    "wurtzite": [(2, 6), (2, 6)],
    "zincblende": [(1, 24), (1, 24)],
    "diamond": [(2, 24)],
    "pm3m_64": [(48, 1), (12, 4), (3, 16), (1, 48)],
}


def cubic_point_group():
    """The 48 signed permutation matrices."""
    out = []
    for p in itertools.permutations(range(3)):
        for s in itertools.product((1, -1), repeat=3):
            M = np.zeros((3, 3))
            for r in range(3):
                M[r, p[r]] = s[r]
            out.append(M)
    return out


def orbit_of(point):
    pts = []
    for M in cubic_point_group():
        q = (np.asarray(point, np.float64) @ M) % 1.0
        q = np.where(np.abs(q - 1.0) < 1e-12, 0.0, q)
        if not any(np.abs((q - p) - np.round(q - p)).max() < 1e-9 for p in pts):
            pts.append(q)
    return pts


def pm3m_64():
    """Pm-3m, edge 10 A, four species: the general orbit of (0.11, 0.23, 0.37), the orbits of (0.17, 0.17, 0) and (1/2, 1/2, 0), the origin."""
    z, f = [], []
    for species, point, count in ((8, (0.11, 0.23, 0.37), 48), (14, (0.17, 0.17, 0.0), 12), (26, (0.5, 0.5, 0.0), 3), (56, (0.0, 0.0, 0.0), 1)):
        pts = orbit_of(point)
        assert len(pts) == count
        z += [species] * count
        f += pts
    return np.eye(3) * 10.0, z, np.array(f)


def one_atom_cubic():
    return np.eye(3) * 3.3, [29], np.zeros((1, 3))


def base(name):
    return pm3m_64() if name == "pm3m_64" else C.known_crystals()[name][0]


def perturb(rng, crystal):
    """Every atom moved by a vector drawn uniformly from the ball of radius MOVE (A); the cell strained by a symmetric matrix with entries
    drawn uniformly from [-STRAIN, STRAIN]."""
    L, z, f = crystal
    L, f = np.asarray(L, np.float64), np.asarray(f, np.float64)
    e = rng.uniform(-STRAIN, STRAIN, (3, 3))
    e = (e + e.T) / 2
    L2 = L @ (np.eye(3) + e)
    d = rng.normal(size=f.shape)
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * (MOVE * rng.uniform(0, 1, (len(f), 1)) ** (1.0 / 3.0))
    return L2, list(z), (f + d @ np.linalg.inv(L)) % 1.0


@lru_cache(maxsize=None)
def perturbed():
    """name -> the perturbed crystal, one generator in the order of PERTURBED."""
    rng = np.random.default_rng(SEED)
    return {name: perturb(rng, base(name)) for name in PERTURBED}


@lru_cache(maxsize=None)
def transformed():
    """name -> (crystal, perm): the perturbed crystal under a unimodular change of basis, an origin shift, an atom permutation (and a rigid
    rotation, which no output but the cell's orientation sees); atom i of the copy is atom perm[i] of the original."""
    rng = np.random.default_rng(SEED + 1)
    out = {}
    for name, crystal in perturbed().items():
        copy, perm, *_ = K.transformed(rng, crystal, scale=1.0, return_parts=True)
        out[name] = (copy, [int(v) for v in perm])
    return out


AMBIGUOUS_CRYSTAL = (np.eye(3) * 4.0, [29, 29], np.array([[0, 0, 0], [0.012, 0, 0]], np.float64))   # two atoms of a species 0.05 A apart
GUARD_NAMES = ("rutile~", "nan_lattice", "flat_cell", "sc_444", "ambiguous", "rocksalt_conv~")


def guard_batch():
    """Perturbed rutile, a NaN lattice, a flat cell, the 4 x 4 x 4 supercell (more operations than the cap), an ambiguous crystal, perturbed
    rock salt: (offsets, types, frac, lat)."""
    p = perturbed()
    flat = (np.array([[4.0, 0, 0], [0, 4.0, 0], [4.0, 4.0, 0]]), [29, 8], np.array([[0, 0, 0], [.5, .5, .5]]))
    off, types, frac, lat = K.batch([p["rutile"], K.cell("rocksalt_prim"), flat, C.sc_supercell_444(), AMBIGUOUS_CRYSTAL, p["rocksalt_conv"]])
    lat = lat.copy()
    lat[1, 4] = np.nan
    return off, types, frac, lat


def regular_crystals():
    """[(name, crystal)]: the known crystals, the 64-atom cell, the one-atom cube, the perturbed crystals and their transformed copies."""
    out = [(name, v[0]) for name, v in C.known_crystals().items()] + [("pm3m_64", pm3m_64()), ("one_atom_cubic", one_atom_cubic())]
    out += [(name + "~", c) for name, c in perturbed().items()]
    out += [(name + "~T", c) for name, (c, _) in transformed().items()]
    return out


@lru_cache(maxsize=None)
def regular_results(fill=0):
    """(names, batch, chain) of regular_crystals() and the random set under the restatement."""
    named = regular_crystals()
    crystals = [c for _, c in named] + C.random_set()
    batch = K.batch(crystals)
    return [n for n, _ in named] + ["random%d" % i for i in range(len(crystals) - len(named))], batch, V.chain(batch, SYMPREC, K.COS_TOL, fill=fill)


@lru_cache(maxsize=None)
def guard_results(fill=0):
    batch = guard_batch()
    return batch, V.chain(batch, SYMPREC, K.COS_TOL, fill=fill)


def batch_300():
    """300 crystals of 1 .. 3 atoms with perturbed rock salt at positions 0, 150 and 299."""
    rng = np.random.default_rng(67)
    small = [K.random_crystal(rng, c) for c in ([1], [2], [1, 2])]
    crystals = [small[i % 3] for i in range(300)]
    for pos in (0, 150, 299):
        crystals[pos] = perturbed()["rocksalt_conv"]
    return crystals
