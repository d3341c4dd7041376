"""The structure fingerprint of include/matinvent_hip_fp.h restated in numpy: float64 without truncation (every bin of every
pair-image within r_max + 12 sigma + one bin receives its Gaussian mass; beyond that the mass is below 1e-30) and with a reach taken
generously from the perpendicular heights, and the same formulas in float32 for error budgets.  Also the kernel's verdict (status, species
count, translations per pair) restated, a brute-force element-by-element evaluation for tiny cells, the re-descriptions of a crystal the
fingerprint must not see, and the test crystals shared by the CPU and GPU tests."""
import math

import numpy as np
import torch

R_MAX, NBINS, SIGMA = 8.0, 64, 0.15
CUT, MAX_SPECIES, MAX_BLOCKS, MAX_BINS, MAX_REACH, MIN_VOLUME = 6.0, 8, 36, 64, 16, 0.1   # include/matinvent_hip_fp.h
OK, SPECIES, NONFINITE, VOLUME, REACH, ATOMS = 0, 1, 2, 3, 4, 5
TAIL = 12.0   # the restatement's own horizon in sigma: erfc(12 / sqrt 2) / 2 < 1e-32
# what one contribution can lose in the kernel: the tail beyond CUT sigma on either side, and the floor of its 2^-32 fixed-point quantum per bin
JUMP = 0.5 * math.erfc(CUT / math.sqrt(2.0))
QUANTUM = 2.0 ** -32


def _heights(L):
    L = np.asarray(L, np.float64).reshape(3, 3)
    cn = np.array([np.linalg.norm(np.cross(L[1], L[2])), np.linalg.norm(np.cross(L[2], L[0])), np.linalg.norm(np.cross(L[0], L[1]))])
    V = abs(float(np.dot(L[0], np.cross(L[1], L[2]))))
    return V, cn


def verdict(types, frac, L, r_max=R_MAX, sigma=SIGMA):
    """(status, species count, translations visited per pair) as the kernel decides them; `margin` is how far the nearest decision
    (volume threshold, reach limit, the ceil of a reach) is from flipping, so that a test can keep its cells away from fp32 ties."""
    types, frac, L = np.asarray(types).reshape(-1), np.asarray(frac, np.float64).reshape(-1, 3), np.asarray(L, np.float64).reshape(3, 3)
    m = len(set(int(z) for z in types if 1 <= int(z) <= 100))
    if len(types) == 0 or any(not 1 <= int(z) <= 100 for z in types):
        return ATOMS, m, 0.0, 1.0
    if not (np.isfinite(L).all() and np.isfinite(frac).all()):
        return NONFINITE, m, 0.0, 1.0
    V, cn = _heights(L)
    if not (np.isfinite(V) and np.isfinite(cn).all()):
        return NONFINITE, m, 0.0, 1.0
    if not V >= MIN_VOLUME:
        return VOLUME, m, 0.0, abs(V - MIN_VOLUME)
    x = (r_max + CUT * sigma) * cn / V * 1.00001 + 0.5
    if not (x <= MAX_REACH).all():
        return REACH, m, 0.0, float(np.abs(x - MAX_REACH).min())
    reach = np.ceil(x)
    margin = float(np.minimum(reach - x, x - (reach - 1)).min())
    return (SPECIES if m > MAX_SPECIES else OK), m, float(np.prod(2 * reach + 1)), margin


def _blocks(types):
    zs = sorted(set(int(z) for z in types))
    slot = {z: k for k, z in enumerate(zs)}
    m = len(zs)
    na = [int((np.asarray(types) == z).sum()) for z in zs]
    return zs, slot, m, na


def fingerprint(types, frac, L, r_max=R_MAX, nbins=NBINS, sigma=SIGMA, dtype=np.float64):
    """dict(u [36 nbins], status, m, norm, images, g, dg_unit): u is the unit row (zeros when flagged); dg_unit is, per element, what ONE
    count of error in every contribution that can reach the element's bin would do to g: the number of the block's pair-images with
    |R - R_k| <= D / 2 + TAIL sigma (the others hold less than 1e-32 of a count there), over the shell volume, times sqrt w.  `floor()`
    scales it."""
    types = np.asarray(types).reshape(-1)
    status, m, images, _ = verdict(types, frac, L, r_max, sigma)
    out = dict(u=np.zeros(MAX_BLOCKS * nbins, dtype), status=status, m=m, norm=0.0, images=images)
    if status != OK:
        return out
    dt = np.dtype(dtype)
    tdt = torch.float64 if dt == np.float64 else torch.float32
    n = len(types)
    zs, slot, m, na = _blocks(types)
    x = np.asarray(frac, dt).reshape(n, 3)
    x = x - np.floor(x)
    Lm = np.asarray(L, dt).reshape(3, 3)
    V64, cn = _heights(L)
    horizon = r_max + TAIL * sigma + r_max / nbins
    reach = np.ceil(horizon * cn / V64 + 1.0).astype(int)          # wrapped coordinates: differences in (-1, 1)
    ta, tb, tc = (np.arange(-r, r + 1) for r in reach)
    T = np.stack(np.meshgrid(ta, tb, tc, indexing="ij"), -1).reshape(-1, 3)
    home = int(np.where((T == 0).all(1))[0][0])
    d = x[None, :, :] - x[:, None, :]                               # [i, j] = x_j - x_i
    sl = np.array([slot[int(z)] for z in types])
    bi, bj = np.meshgrid(sl, sl, indexing="ij")
    keep_pair = bi <= bj
    blk_of = bi * m - bi * (bi - 1) // 2 + (bj - bi)
    nblk = m * (m + 1) // 2
    D = dt.type(r_max) / dt.type(nbins)
    edges = np.arange(nbins + 1).astype(dt) * D
    inv = dt.type(1.0) / (dt.type(sigma) * dt.type(math.sqrt(2.0)))
    C = np.zeros((nblk, nbins), dt)
    P = np.zeros((nblk, nbins))
    Rk64 = (np.arange(nbins) + 0.5) * (r_max / nbins)
    chunk = max(1, int(4e6 // max(1, n * n)))
    for t0 in range(0, len(T), chunk):
        Tc = T[t0:t0 + chunk].astype(dt)
        fr = d[:, :, None, :] + Tc[None, None, :, :]
        cart = fr @ Lm
        R = np.sqrt((cart * cart).sum(-1))                          # [i, j, t]
        ok = (R < horizon) & keep_pair[:, :, None]
        if t0 <= home < t0 + chunk:
            ok[np.arange(n), np.arange(n), home - t0] = False       # (i, i, 0) is not a pair
        ii, jj, tt = np.nonzero(ok)
        if len(ii) == 0:
            continue
        Rs, bs = R[ii, jj, tt], blk_of[ii, jj]
        E = torch.erf(torch.from_numpy(((edges[None, :] - Rs[:, None]) * inv).astype(dt)).to(tdt)).numpy()
        mass = dt.type(0.5) * (E[:, 1:] - E[:, :-1])
        for b in range(nblk):
            sel = bs == b
            if sel.any():
                C[b] += mass[sel].sum(0, dtype=dt)
                P[b] += (np.abs(Rs[sel].astype(np.float64)[:, None] - Rk64[None, :]) <= 0.5 * r_max / nbins + TAIL * sigma).sum(0)
    g = np.zeros(MAX_BLOCKS * nbins, dt)
    dg = np.zeros(MAX_BLOCKS * nbins)
    Rk = (np.arange(nbins).astype(dt) + dt.type(0.5)) * D
    V = dt.type(abs(np.linalg.det(Lm.astype(np.float64)))) if dt == np.float64 else np.float32(V64)
    b = 0
    for p in range(m):
        for q in range(p, m):
            nab = dt.type(na[p] * na[q])
            shell = (dt.type(4.0 * math.pi) * Rk * Rk * D) * nab / V
            w = dt.type(2.0 if p < q else 1.0) * nab / dt.type(n * n)
            g[b * nbins:(b + 1) * nbins] = np.sqrt(w) * (C[b] / shell - dt.type(1.0))
            dg[b * nbins:(b + 1) * nbins] = math.sqrt(float(w)) * P[b] / shell.astype(np.float64)
            b += 1
    norm = float(np.sqrt((g.astype(np.float64) ** 2).sum())) if dt == np.float64 else float(np.sqrt((g * g).sum(dtype=dt)))
    out.update(u=(g / dt.type(norm)).astype(dt), norm=norm, g=g, dg_unit=dg)
    return out


def floor(ref, per_contribution=JUMP + QUANTUM):
    """Per element of u: the first-order effect of an error of `per_contribution` counts in every contribution that reaches a bin (the
    kernel drops at most JUMP of a contribution from a bin, and rounds what it adds down by less than QUANTUM) -- on the
    element itself, delta g_e / ||g||, and through the norm, |u_e| ||delta g|| / ||g||."""
    dg = ref["dg_unit"] * per_contribution
    return dg / ref["norm"] + np.abs(ref["u"].astype(np.float64)) * float(np.sqrt((dg * dg).sum())) / ref["norm"]


def distance(u1, u2):
    return 0.5 * (1.0 - float(np.dot(np.asarray(u1, np.float64), np.asarray(u2, np.float64))))


def brute(types, frac, L, r_max, nbins, sigma, reach):
    """Element by element, math.erf, python loops: for tiny cells only."""
    types = [int(z) for z in types]
    zs, slot, m, na = _blocks(types)
    n = len(types)
    L = np.asarray(L, np.float64).reshape(3, 3)
    V = abs(np.linalg.det(L))
    D = r_max / nbins
    g = np.zeros(MAX_BLOCKS * nbins)
    b = 0
    for p in range(m):
        for q in range(p, m):
            for k in range(nbins):
                Rk = (k + 0.5) * D
                c = 0.0
                for i in range(n):
                    for j in range(n):
                        if slot[types[i]] != p or slot[types[j]] != q:
                            continue
                        for a1 in range(-reach, reach + 1):
                            for a2 in range(-reach, reach + 1):
                                for a3 in range(-reach, reach + 1):
                                    if i == j and a1 == 0 and a2 == 0 and a3 == 0:
                                        continue
                                    v = (np.asarray(frac[j], np.float64) - np.asarray(frac[i], np.float64) + np.array([a1, a2, a3])) @ L
                                    R = math.sqrt(float(v @ v))
                                    c += 0.5 * (math.erf((Rk + D / 2 - R) / (sigma * math.sqrt(2))) - math.erf((Rk - D / 2 - R) / (sigma * math.sqrt(2))))
                F = c / (4 * math.pi * Rk * Rk * D * na[p] * na[q] / V) - 1.0
                g[b * nbins + k] = math.sqrt((2.0 if p < q else 1.0) * na[p] * na[q] / n ** 2) * F
            b += 1
    return g / math.sqrt(float(g @ g))


# ---- re-descriptions of one crystal ---------------------------------------------------------------------------------------------------
def permuted(c, seed=0):
    t, x, L = c
    p = np.random.default_rng(seed).permutation(len(t))
    return np.asarray(t)[p], np.asarray(x)[p], L


def translated(c, shift=(0.37, -0.61, 0.123)):
    t, x, L = c
    y = np.asarray(x, np.float64) + np.asarray(shift)
    return t, y - np.floor(y), L


UNIMODULAR = np.array([[1, 1, 0], [0, 1, 0], [1, 0, 1]], np.float64)   # det 1


def rebased(c, U=UNIMODULAR):
    """L' = U L, x' = x U^-1: the same lattice and the same atoms in another basis."""
    t, x, L = c
    y = np.asarray(x, np.float64) @ np.linalg.inv(U)
    return t, y - np.floor(y), U @ np.asarray(L, np.float64)


def supercell(c):
    """2 x 1 x 1."""
    t, x, L = c
    x = np.asarray(x, np.float64)
    x2 = np.concatenate([x * [0.5, 1, 1], x * [0.5, 1, 1] + [0.5, 0, 0]])
    return np.concatenate([t, t]), x2, np.asarray(L, np.float64) * [[2.0], [1.0], [1.0]]


REDESCRIPTIONS = (("permutation", permuted), ("translation", translated), ("basis", rebased), ("supercell", supercell))


# ---- crystals ---------------------------------------------------------------------------------------------------------------------------
def rock_salt(a=4.2, za=11, zb=17):
    """AB, conventional cell of 8 atoms."""
    fcc = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
    return np.array([za] * 4 + [zb] * 4), np.concatenate([fcc, fcc + [.5, .5, .5]]) % 1.0, np.eye(3) * a


def cscl_type(a=3.3, za=11, zb=17):
    """AB, 2 atoms, nearly the volume per formula unit of rock_salt(4.2) / 4 x 2."""
    return np.array([za, zb]), np.array([[0, 0, 0], [.5, .5, .5]]), np.eye(3) * a


def random_crystal(n, species, seed, L=None, volume_per_atom=14.0):
    g = np.random.default_rng(seed)
    if L is None:
        a = (n * volume_per_atom) ** (1 / 3)
        L = np.eye(3) * a + 0.08 * a * g.standard_normal((3, 3))
    sp = np.asarray(species)
    t = np.concatenate([sp, g.choice(sp, n - len(sp))]) if n >= len(sp) else sp[:n]
    return t.astype(np.int64), g.random((n, 3)), np.asarray(L, np.float64)


SKEWED = np.array([[3.0, 0.0, 0.0], [5.5, 2.4, 0.0], [0.3, 0.2, 5.0]])   # edge b = 6.0 A, perpendicular height along b = 2.4 A


def kernel_cases():
    """name -> (types, frac, lattice): the cases of the kernel-against-float64 comparison."""
    e8, e9 = [3, 8, 11, 13, 14, 17, 26, 29], [3, 8, 11, 13, 14, 17, 26, 29, 47]
    return {
        "one_atom": (np.array([26]), np.array([[0.2, 0.7, 0.4]]), np.eye(3) * 3.1 + 0.1),
        "two_atoms": random_crystal(2, [3, 8], 1),
        "five_atoms": random_crystal(5, [3, 8], 2),
        "eighty_six": random_crystal(86, [3, 8, 26], 3),
        "one_seven_one": random_crystal(171, [8, 14], 4),
        "eight_species": random_crystal(12, e8, 5),
        "nine_species": random_crystal(12, e9, 6),
        "cubic_2p5": (np.array([29]), np.array([[0.0, 0.0, 0.0]]), np.eye(3) * 2.5),
        "skewed": (np.array([3, 3, 8]), np.array([[0.1, 0.2, 0.3], [0.6, 0.7, 0.1], [0.4, 0.9, 0.8]]), SKEWED),
        "cell_12": random_crystal(6, [11, 17], 7, L=np.eye(3) * 12.0),
    }


def flagged_cases():
    t, x = np.array([3, 8]), np.array([[0.1, 0.2, 0.3], [0.6, 0.5, 0.4]])
    nan = np.eye(3) * 4.0
    nan[1, 2] = np.nan
    return {
        "nan_lattice": (t, x, nan, NONFINITE),
        "tiny_volume": (t, x, np.eye(3) * 0.4, VOLUME),                                     # V = 0.064
        "collapsed": (t, x, np.array([[6.0, 0, 0], [0, 6.0, 0], [0, 0, 0.2]]), REACH),      # V = 7.2, height 0.2 along c
    }
