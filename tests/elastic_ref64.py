"""A numpy float64 restatement of the elasticity kernels (include/matinvent_hip_elastic.h, matinvent_amd/csrc/elastic_fit.h),
operation for operation in the header's order -- every product and every sum rounded separately, every sum a serial loop in a fixed order
-- so that the device can be held to it bit for bit; and a synthetic energy of minimum-image springs with an analytic lattice gradient and
an analytic clamped-ion stress derivative to feed it.  The eigenvalues are tests/vib_ref64.py's Jacobi.  Plain numpy, no GPU."""
import numpy as np

from tests import vib_ref64 as V

OK, BAD_INPUT, SINGULAR = 0, 1, 2
COPIES, ROW = 13, 8
GPA = 160.2176634
RELAX_CONVERGED, RELAX_FAILED, RELAX_EXHAUSTED = 1, 2, 3
VOIGT_AXES = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))
AVERAGES = ("voigt", "reuss", "hill")
NAN = float("nan")


# ---- step 1: the strained copies ---------------------------------------------------------------------------------------------------------------

def lattice_ok(lat32, det_min):
    return V.lattice_inverse(lat32, det_min)[0]


def det3(L):
    L = np.asarray(L, np.float64).reshape(9)
    c0, c1, c2 = L[4] * L[8] - L[5] * L[7], L[5] * L[6] - L[3] * L[8], L[3] * L[7] - L[4] * L[6]
    return (L[0] * c0 + L[1] * c1) + L[2] * c2


def strain(lat32, c, h, det_min=1e-3):
    """The float32 lattice [3][3] of copy c: L (I + eps) formed in float64 and rounded once; a bad lattice is copied as it is."""
    lat = np.array(lat32, np.float32, copy=True).reshape(3, 3)
    if c >= 12 or not lattice_ok(lat, det_min):
        return lat
    a, b = VOIGT_AXES[c >> 1]
    hs = -h if c & 1 else h
    e = hs if a == b else 0.5 * hs
    out = lat.copy()
    for q, k in ((a, b), (b, a)):
        out[:, q] = (lat[:, q].astype(np.float64) + lat[:, k].astype(np.float64) * e).astype(np.float32)
    return out


def strain_matrix(c, h):
    """I + eps of copy c, exact."""
    F = np.eye(3)
    if c < 12:
        a, b = VOIGT_AXES[c >> 1]
        hs = -h if c & 1 else h
        if a == b:
            F[a, a] += hs
        else:
            F[a, b] += 0.5 * hs
            F[b, a] += 0.5 * hs
    return F


# ---- step 2: the stress rows ---------------------------------------------------------------------------------------------------------------------

def stress_row(lat32, g_lat32, scale, per_atom, n, det_min=1e-3, ist=RELAX_CONVERGED):
    """(row [8], asym) of one copy from its float32 lattice and lattice gradient."""
    lat32 = np.asarray(lat32, np.float32).reshape(3, 3)
    if ist == RELAX_FAILED or not lattice_ok(lat32, det_min):
        return np.full(ROW, np.nan), NAN
    s = scale * float(n) if per_atom else scale
    L = lat32.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        G = s * np.asarray(g_lat32, np.float32).reshape(3, 3).astype(np.float64)
        T = np.empty((3, 3))
        for i in range(3):
            for j in range(3):
                T[i, j] = (L[0, i] * G[0, j] + L[1, i] * G[1, j]) + L[2, i] * G[2, j]
        Vol = abs(det3(L))
        V2 = 2.0 * Vol
        row = np.array([(T[a, b] + T[b, a]) / V2 for a, b in VOIGT_AXES] + [Vol, 1.0 if ist == RELAX_EXHAUSTED else 0.0])
        mt, md = 0.0, 0.0
        for i in range(3):
            for j in range(3):
                x, y = abs(T[i, j]), abs(T[i, j] - T[j, i])
                mt, md = (x if x > mt else mt), (y if y > md else md)
    return row, (md / mt if mt > 0.0 else 0.0)


# ---- step 3: the fit -----------------------------------------------------------------------------------------------------------------------------

def invert6(Cm):
    """(ok, S) by Gauss-Jordan elimination with partial pivoting, ties to the lowest row."""
    aug = np.concatenate([np.array(Cm, np.float64).reshape(6, 6), np.eye(6)], axis=1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(6):
            piv, best = k, abs(aug[k, k])
            for r in range(k + 1, 6):
                v = abs(aug[r, k])
                if v > best:
                    best, piv = v, r
            p = aug[piv, k]
            if not np.isfinite(p) or p == 0.0:
                return False, np.full((6, 6), np.nan)
            if piv != k:
                aug[[k, piv]] = aug[[piv, k]]
            aug[k] = aug[k] / p
            for i in range(6):
                if i != k:
                    aug[i] = aug[i] - aug[i, k] * aug[k]
    return True, aug[:, 6:].copy()


def _sums(M):
    return (M[0, 0] + M[1, 1]) + M[2, 2], (M[0, 1] + M[0, 2]) + M[1, 2], (M[3, 3] + M[4, 4]) + M[5, 5]


def _derived(K, G):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        K, G = np.float64(K), np.float64(G)
        d = 3.0 * K + G
        return [K, G, ((9.0 * K) * G) / d, (3.0 * K - 2.0 * G) / (2.0 * d), K / G]


def moduli(Cm, S, has_S):
    """[3][5]: Voigt, Reuss, Hill x K, G, E, nu, K / G."""
    out = np.full((3, 5), np.nan)
    a, b, c = _sums(Cm)
    out[0] = _derived((a + 2.0 * b) / 9.0, ((a - b) + 3.0 * c) / 15.0)
    if has_S:
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            a, b, c = _sums(S)
            out[1] = _derived(np.float64(1.0) / (a + 2.0 * b), np.float64(15.0) / ((4.0 * a - 4.0 * b) + 3.0 * c))
            out[2] = _derived((out[0, 0] + out[1, 0]) * 0.5, (out[0, 1] + out[1, 1]) * 0.5)
    return out


def fit(rows, asym, h):
    """Every output of mi_elastic_fit for one crystal from its rows [13][8] and the collect step's asym; C_raw (before the symmetrisation)
    is extra."""
    rows = np.asarray(rows, np.float64).reshape(COPIES, ROW)
    if not np.isfinite(rows).all():
        return dict(C=np.full((6, 6), np.nan), S=np.full((6, 6), np.nan), stress0=np.full(6, np.nan), pressure=NAN, asym=NAN, asym_C=NAN,
                    moduli=np.full((3, 5), np.nan), evals=np.full(6, np.nan), cond=NAN, n_negative=-1, n_unrelaxed=-1, status=BAD_INPUT,
                    C_raw=np.full((6, 6), np.nan))
    A = ((rows[0:12:2, :6] - rows[1:12:2, :6]).T / (2.0 * h)) * GPA
    mc, md = np.abs(A).max(), np.abs(A - A.T).max()
    asym_C = md / mc if mc > 0.0 else 0.0
    Cm = (A + A.T) * 0.5
    r0 = rows[12]
    stress0 = r0[:6] * GPA
    pressure = -(((r0[0] + r0[1]) + r0[2]) * GPA) / 3.0
    has_S, S = invert6(Cm)
    ev, _, _ = V.jacobi(Cm)
    lam = np.abs(ev)
    with np.errstate(invalid="ignore", divide="ignore"):
        cond = float(np.float64(lam.max()) / np.float64(lam.min()))
    return dict(C=Cm, S=S, stress0=stress0, pressure=pressure, asym=asym, asym_C=asym_C, moduli=moduli(Cm, S, has_S), evals=ev, cond=cond,
                n_negative=int((ev < 0.0).sum()), n_unrelaxed=int((rows[:, 7] != 0.0).sum()), status=OK if has_S else SINGULAR, C_raw=A)


FIT_KEYS = ("C", "S", "stress0", "pressure", "asym", "asym_C", "moduli", "evals", "cond", "n_negative", "n_unrelaxed", "status")


# ---- the synthetic energy ------------------------------------------------------------------------------------------------------------------------

def make_springs(n, seed, cell=6.0, grid=False, flat=False):
    """A crystal of n atoms whose energy is a sum of springs 1/2 (d - d0)^T K (d - d0), d = u L: one per pair of atoms with
    u = w(x_j - x_i), w(t) = t - round(t) (the minimum image), and three that tie the cell to itself, u = e_a; K symmetric positive definite,
    d0 the spring's vector in the starting cell stretched by up to 5 %.  The coordinates lie within 1/8 of the cell's centre, so every
    component of u is at most 1/4: a quarter cell from the wrap of w at 1/2, and a strain moves no coordinate.  grid: the lattice elements are
    multiples of 2^-6 below 16, so that L (I + eps) is exact in float32 for h = 2^-5 and 2^-6.  flat: a lattice-independent energy (no
    spring at all)."""
    rng = np.random.default_rng(seed)
    frac = (0.5 + rng.uniform(-0.125, 0.125, (n, 3))).astype(np.float32)
    lat = np.eye(3) * rng.uniform(0.8 * cell, 1.2 * cell, 3)[:, None] + 0.3 * rng.uniform(-1, 1, (3, 3))
    if grid:
        lat = np.round(lat * 64.0) / 64.0
    lat = lat.astype(np.float32)
    x = frac.astype(np.float64)
    i, j = np.triu_indices(n, 1)
    t = x[j] - x[i]
    u = np.concatenate([t - np.round(t), np.eye(3)]) if not flat else np.zeros((0, 3))
    S = len(u)
    a = rng.uniform(-1, 1, (S, 3, 3))
    K = a @ a.transpose(0, 2, 1) + np.eye(3) * rng.uniform(0.2, 2.0, (S, 1, 1))
    d0 = (u @ lat.astype(np.float64)) * (1.0 + 0.05 * rng.uniform(-1, 1, (S, 3)))
    return dict(n=n, frac=frac, lat=lat, u=u, K=K, d0=d0)


def spring_lattice_gradient(sp, lat):
    """(E, dE / dL [3][3]) in float64 at lattice `lat` (any precision, read as float64) and the crystal's own fractional coordinates."""
    L = np.asarray(lat, np.float64).reshape(3, 3)
    if not np.isfinite(L).all():
        return NAN, np.full((3, 3), np.nan)
    r = sp["u"] @ L - sp["d0"]
    f = np.einsum("sa,sab->sb", r, sp["K"])
    return 0.5 * np.einsum("sa,sa->", r, f), sp["u"].T @ f


def spring_copies(sp, h, lat_of_copy=None):
    """The float32 lattice gradients [13][3][3] of the strained copies: the float64 analytic gradient at each copy's float32 lattice (from
    `strain`, or lat_of_copy [13][3][3] -- the device's), rounded."""
    out = np.empty((COPIES, 3, 3), np.float32)
    for c in range(COPIES):
        L = strain(sp["lat"], c, h) if lat_of_copy is None else lat_of_copy[c]
        with np.errstate(invalid="ignore", over="ignore"):
            out[c] = spring_lattice_gradient(sp, L)[1].astype(np.float32)
    return out


def _voigt(M):
    return np.array([(M[a, b] + M[b, a]) * 0.5 for a, b in VOIGT_AXES])


def spring_stress_series(sp, j, s=1.0):
    """The Cauchy stress of the crystal under the strain t E_j is a ratio of polynomials, sigma(t) = (p0 + p1 t + p2 t^2) / q(t) with
    q = 1 + t (j < 3) or 1 - t^2 / 4 (shear).  Returns (a1, a3, r): the analytic clamped-ion derivative d sigma / dt at 0 (Voigt [6],
    eV / A^3, times s), and the exact central difference (sigma(h) - sigma(-h)) / (2 h) = a1 + a3 h^2 / (1 - r h^2)."""
    L = sp["lat"].astype(np.float64)
    a, b = VOIGT_AXES[j]
    E = np.zeros((3, 3))
    E[a, b] += 0.5
    E[b, a] += 0.5
    D = sp["u"] @ L
    f0 = np.einsum("sa,sab->sb", D - sp["d0"], sp["K"])
    DE = D @ E
    fE = np.einsum("sa,sab->sb", DE, sp["K"])
    Vol = abs(np.linalg.det(L))
    p0, p1, p2 = (s * _voigt(M) / Vol for M in (D.T @ f0, DE.T @ f0 + D.T @ fE, DE.T @ fE))
    if j < 3:
        return p1 - p0, p1 - p0 - p2, 1.0
    return p1, p1 * 0.25, 0.25


def analyze(sp, h, scale=1.0, per_atom=False, det_min=1e-3, g_copies=None, lats=None, ist=None):
    """Steps 1 to 3 of one synthetic crystal: lats [13][3][3] float32, rows [13][8], and every output of the fit."""
    lats = np.stack([strain(sp["lat"], c, h, det_min) for c in range(COPIES)]) if lats is None else lats
    g = spring_copies(sp, h, lats) if g_copies is None else g_copies
    ist = [RELAX_CONVERGED] * COPIES if ist is None else ist
    pairs = [stress_row(lats[c], g[c], scale, per_atom, sp["n"], det_min, ist[c]) for c in range(COPIES)]
    rows = np.stack([p[0] for p in pairs])
    return dict(lats=lats, rows=rows, **fit(rows, pairs[12][1], h))


# ---- the host module's chunk plan (elasticity.chunk_plan restated) ----------------------------------------------------------------------------

def chunk_plan(num_crystals, batch_size):
    """[(source crystal, copy)] in order, cut into chunks of batch_size."""
    flat = [(b, c) for b in range(num_crystals) for c in range(COPIES)]
    return [flat[s:s + batch_size] for s in range(0, len(flat), batch_size)]


# ---- the case file of scripts/elastic_host_check.cpp ------------------------------------------------------------------------------------------

def write_case(path, crystals, g_copies, ists, h, scale, per_atom, det_min):
    with open(path, "wb") as f:
        f.write(np.array([len(crystals), int(per_atom)], np.int32).tobytes() + np.array([h, scale, det_min], np.float64).tobytes())
        for sp, g, ist in zip(crystals, g_copies, ists):
            f.write(np.array([sp["n"]], np.int32).tobytes() + np.asarray(sp["lat"], np.float32).tobytes() + np.asarray(g, np.float32).tobytes())
            f.write(np.asarray(ist, np.int32).tobytes())


def read_out(path, count):
    buf, at, out = open(path, "rb").read(), 0, []

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(buf, dtype, n, at)
        at += a.nbytes
        return a

    for _ in range(count):
        r = dict(lats=take(np.float32, COPIES * 9).reshape(COPIES, 3, 3), rows=take(np.float64, COPIES * ROW).reshape(COPIES, ROW),
                 C=take(np.float64, 36).reshape(6, 6), S=take(np.float64, 36).reshape(6, 6), stress0=take(np.float64, 6),
                 pressure=float(take(np.float64, 1)[0]), asym=float(take(np.float64, 1)[0]), asym_C=float(take(np.float64, 1)[0]),
                 moduli=take(np.float64, 15).reshape(3, 5), evals=take(np.float64, 6), cond=float(take(np.float64, 1)[0]),
                 n_negative=int(take(np.int32, 1)[0]), n_unrelaxed=int(take(np.int32, 1)[0]), status=int(take(np.int32, 1)[0]))
        out.append(r)
    assert at == len(buf)
    return out
