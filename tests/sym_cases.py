"""Inputs shared by the symmetry finder's CPU and GPU tests, built from the cells of tests/sm_cases.py: the known crystals
with their (operations, pure translations, point group), supercells by Hermite normal form, and the restatement's results computed once."""
from functools import lru_cache

import numpy as np

from tests import sm_cases as K
from tests import sm_ref64 as R
from tests import sym_ref64 as S

SYMPREC = 0.1
TETRA = np.diag([4.6, 4.6, 2.96])


def known_crystals():
    """name -> (crystal, n_ops, n_trans, point group)."""
    rng = np.random.default_rng(17)
    u = 0.305
    tri = K.random_crystal(rng, [2, 1])
    half = rng.uniform(0.05, 0.45, (3, 3))
    paired = (K.triclinic(rng, 1.2), [8, 14, 14, 8, 14, 14], np.concatenate([half, 1.0 - half]))
    base = K.random_crystal(rng, [2, 1])
    out = {
        "sc": (K.cell("sc"), 48, 1, "m-3m"),
        "fcc": (K.cell("fcc"), 48, 1, "m-3m"),
        "bcc": (K.cell("bcc"), 48, 1, "m-3m"),
        "diamond": ((K.FCC, [6, 6], np.array([[0, 0, 0], [.25, .25, .25]])), 48, 1, "m-3m"),
        "zincblende": ((K.FCC, [30, 16], np.array([[0, 0, 0], [.25, .25, .25]])), 24, 1, "-43m"),
        "rocksalt_conv": (K.cell("rocksalt_conv"), 192, 4, "m-3m"),
        "cscl": (K.cell("cscl"), 48, 1, "m-3m"),
        "hcp": (K.cell("hex2"), 24, 1, "6/mmm"),
        "wurtzite": ((K.HEX, [30, 30, 16, 16], np.array([[1 / 3, 2 / 3, 0], [2 / 3, 1 / 3, .5], [1 / 3, 2 / 3, .375], [2 / 3, 1 / 3, .875]])), 12, 1, "6mm"),
        "rutile": ((TETRA, [22, 22, 8, 8, 8, 8], np.array([[0, 0, 0], [.5, .5, .5], [u, u, 0], [1 - u, 1 - u, 0], [.5 + u, .5 - u, .5], [.5 - u, .5 + u, .5]])),
                   16, 1, "4/mmm"),
        "triclinic": (tri, 1, 1, "1"),
        "triclinic_inversion": (paired, 2, 1, "-1"),
        "triclinic_2x1x1": (supercell(base, [[2, 0, 0], [0, 1, 0], [0, 0, 1]]), 2, 2, "1"),
    }
    return {k: ((np.asarray(c[0], np.float64), list(c[1]), np.asarray(c[2], np.float64)), a, b, g) for k, (c, a, b, g) in out.items()}


def hnf_matrices(index):
    """Every 3 x 3 Hermite normal form (lower triangular, 0 <= below-diagonal < the row's diagonal) of determinant `index`."""
    out = []
    for a in range(1, index + 1):
        if index % a:
            continue
        for c in range(1, index // a + 1):
            if (index // a) % c:
                continue
            f = index // a // c
            for b in range(c):
                for d in range(f):
                    for e in range(f):
                        out.append([[a, 0, 0], [b, c, 0], [d, e, f]])
    return out


def supercell(crystal, H):
    """The supercell of basis H x L: every atom at the |det H| lattice points of the old lattice inside the new cell."""
    L, z, f = crystal
    L, f, H = np.asarray(L, np.float64), np.asarray(f, np.float64).reshape(-1, 3), np.asarray(H, np.int64)
    Hinv = np.linalg.inv(H.astype(np.float64))
    det = int(round(abs(np.linalg.det(H))))
    span = int(np.abs(H).sum()) + 1
    grid = np.stack(np.meshgrid(*[np.arange(-span, span + 1)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    inside = grid @ Hinv
    pts = list(grid[((inside > -1e-9) & (inside < 1 - 1e-9)).all(axis=1)])
    assert len(pts) == det
    zs, fs = [], []
    for a in range(len(z)):
        for p in pts:
            zs.append(z[a])
            fs.append(((f[a] + p) @ Hinv) % 1.0)
    return H.astype(np.float64) @ L, zs, np.array(fs)


def sc_supercell_444():
    L, z, f = K.cell("sc")
    return supercell((L, z, f), np.diag([4, 4, 4]))


def random_set(seed=23):
    """Random crystals of 1, 2, 3, 8, 20 (three species, the rarest 4), 33 and 64 atoms."""
    rng = np.random.default_rng(seed)
    return [K.random_crystal(rng, c) for c in ([1], [2], [1, 2], [5, 3], [9, 4, 7], [20, 13], [64])]


def analyse(crystals, symprec=SYMPREC, fill=0, margin=True):
    """(batch, prepared, tol, find, primitive) under the restatement."""
    batch = K.batch(crystals)
    P = R.prepare(*batch)
    tol = S.tolerances(batch[0], batch[3], symprec)
    F = S.find(P, tol, K.COS_TOL, fill=fill, margin=margin)
    return batch, P, tol, F, S.primitive(P, batch[1], batch[2], batch[3], F, fill=fill, margin=margin)


@lru_cache(maxsize=None)
def known_results():
    known = known_crystals()
    return known, analyse([v[0] for v in known.values()])


@lru_cache(maxsize=None)
def capped_results():
    return analyse([sc_supercell_444()])


@lru_cache(maxsize=None)
def random_results():
    crystals = random_set()
    return crystals, analyse(crystals)
