"""Inputs shared by the structure matcher's CPU and GPU tests: named cells, random crystals, transformed copies and the batch
layout of mi_sm_prepare.  A crystal is (lattice [3, 3] rows are cell vectors, atomic numbers [n], fractional coordinates [n, 3])."""
import math

import numpy as np

A0 = 4.0
FCC = np.array([[0, .5, .5], [.5, 0, .5], [.5, .5, 0]]) * A0
BCC = np.array([[-.5, .5, .5], [.5, -.5, .5], [.5, .5, -.5]]) * A0
HEX = np.array([[1, 0, 0], [-.5, math.sqrt(3) / 2, 0], [0, 0, 1.6]]) * 3.0
CELLS = {
    "sc": (np.eye(3) * A0, [29], [[0, 0, 0]]),
    "fcc": (FCC, [29], [[0, 0, 0]]),
    "bcc": (BCC, [26], [[0, 0, 0]]),
    "rocksalt_prim": (FCC, [11, 17], [[0, 0, 0], [.5, .5, .5]]),
    "rocksalt_conv": (np.eye(3) * A0, [11] * 4 + [17] * 4,
                      [[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0], [.5, .5, .5], [.5, 0, 0], [0, .5, 0], [0, 0, .5]]),
    "hex2": (HEX, [12, 12], [[1 / 3, 2 / 3, .25], [2 / 3, 1 / 3, .75]]),
    "cscl": (np.eye(3) * 3.5, [11, 17], [[0, 0, 0], [.5, .5, .5]]),
}
KNOWN_MAPS = {"sc": 48, "fcc": 48, "bcc": 48, "rocksalt_prim": 48, "rocksalt_conv": 48, "hex2": 24}


def cell(name):
    L, z, f = CELLS[name]
    return np.asarray(L, np.float64), list(z), np.asarray(f, np.float64)


def triclinic(rng, scale=1.0):
    """A well-conditioned random triclinic cell: a perturbed orthorhombic box."""
    return (np.diag(rng.uniform(4.0, 7.0, 3)) + rng.uniform(-0.8, 0.8, (3, 3))) * scale


def random_crystal(rng, counts, species=None):
    """counts: atoms per species; atoms in shuffled order."""
    species = species or [3, 8, 26, 14, 30][:len(counts)]
    z = [s for s, k in zip(species, counts) for _ in range(k)]
    order = rng.permutation(len(z))
    n = len(z)
    L = triclinic(rng, (n / 4.0) ** (1 / 3))
    return L, [z[i] for i in order], rng.uniform(0, 1, (n, 3))


def random_unimodular(rng, steps=6):
    U = np.eye(3, dtype=np.int64)
    for _ in range(steps):
        i, j = rng.choice(3, 2, replace=False)
        E = np.eye(3, dtype=np.int64)
        E[i, j] = rng.integers(-1, 2)
        U = E @ U
    return U


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def transformed(rng, crystal, sigma=0.0, scale=None, return_parts=False):
    """A copy under a random atom permutation, rigid translation, unimodular change of basis, rotation and uniform scaling, with Gaussian
    fractional displacements of width sigma."""
    L, z, f = crystal
    L, f = np.asarray(L, np.float64), np.asarray(f, np.float64)
    n = len(z)
    perm = rng.permutation(n)
    U = random_unimodular(rng)
    R = random_rotation(rng)
    s = rng.uniform(0.8, 1.25) if scale is None else scale
    t = rng.uniform(0, 1, 3)
    f2 = (f + t + sigma * rng.normal(size=f.shape)) @ np.linalg.inv(U.astype(np.float64))
    L2 = s * (U @ L) @ R.T
    out = (L2, [z[i] for i in perm], (f2 % 1.0)[perm])
    return (out, perm, U, R, s, t) if return_parts else out


def batch(crystals):
    """(offsets int32 [B + 1], types int32 [N], frac float32 [N, 3], lat float32 [B, 9]): mi_sm_prepare's inputs."""
    off, types, frac, lat = [0], [], [], []
    for L, z, f in crystals:
        off.append(off[-1] + len(z))
        types += list(z)
        frac.append(np.asarray(f, np.float64).reshape(-1, 3))
        lat.append(np.asarray(L, np.float64).reshape(9))
    return (np.asarray(off, np.int32), np.asarray(types, np.int32), np.concatenate(frac).astype(np.float32) if frac else np.zeros((0, 3), np.float32),
            np.stack(lat).astype(np.float32))


COS_TOL = math.cos(math.radians(5.0))


def regular_set(seed=7):
    """The crystals of the regular-path tests: every named cell and a transformed copy of it; 1, 2 and 3 atoms; 20 atoms in 3 species, the
    rarest having 4; 33 atoms; 64 atoms of one species -- each random one beside a displaced, transformed copy.  Returns (crystals, pairs)."""
    rng = np.random.default_rng(seed)
    crystals, pairs = [], []
    for name in CELLS:
        c = cell(name)
        crystals += [c, transformed(rng, c)]
        pairs += [(len(crystals) - 2, len(crystals) - 2), (len(crystals) - 2, len(crystals) - 1)]
    for counts in ([1], [2], [1, 2], [9, 4, 7], [20, 13], [64]):
        c = random_crystal(rng, counts)
        crystals += [c, transformed(rng, c, sigma=0.01)]
        pairs.append((len(crystals) - 2, len(crystals) - 1))
    names = list(CELLS)
    pairs.append((2 * names.index("rocksalt_prim"), 2 * names.index("cscl")))   # rocksalt against CsCl primitive cells
    return crystals, pairs
