"""A numpy float64 restatement of the phonon kernels (include/matinvent_hip_phonon.h, matinvent_amd/csrc/phonon_fc.h), operation
for operation in the header's order -- every product and every sum rounded separately, every sum a serial loop in ascending index order --
so that the device can be held to it bit for bit; and a synthetic harmonic crystal DEFINED BY ITS FORCE CONSTANTS to feed it.  The
eigenvalues, frequencies and thermodynamic terms are tests/vib_ref64.py's; the phase table is phonons.phase_table, the one numpy function
the host hands to the device too.  Plain numpy, no GPU."""
import numpy as np

from matinvent_amd.phonons import MeshPoints, mesh_points, phase_table   # noqa: F401
from tests import vib_ref64 as V

OK, NO_CONVERGENCE, BAD_INPUT = V.OK, V.NO_CONVERGENCE, V.BAD_INPUT
MAX_PRIM, IMAGES = 128, 27
TIE_TOL = 1e-5
TIE_GUARD = 1e-9     # no tie decision of any fixture may lie this close to tie_tol
MODEL_MASSES = (1.008, 15.999, 55.845, 207.2)
SHIFTS = np.array([(s // 9 - 1, (s // 3) % 3 - 1, s % 3 - 1) for s in range(IMAGES)], dtype=np.int64)


def images(reps):
    """[N][3] image triples in make_supercell's (lexicographic) order."""
    return np.array([(a, b, c) for a in range(reps[0]) for b in range(reps[1]) for c in range(reps[2])], dtype=np.int64)


def image_index(trip, reps):
    t = np.asarray(trip, dtype=np.int64) % np.asarray(reps, dtype=np.int64)
    return (t[..., 0] * reps[1] + t[..., 1]) * reps[2] + t[..., 2]


def neg_images(reps):
    """[N]: the index of -I modulo reps."""
    return image_index(-images(reps), reps)


# ---- step 2: force constants ------------------------------------------------------------------------------------------------------------------

def lattice_ok(lat32, det_min):
    return V.lattice_inverse(lat32, det_min)[0]


def image_dists(frac32, lat32, n):
    """[n][Ns][27]: |(x_at - x_i + S) L| in the header's order of operations."""
    x = np.asarray(frac32, np.float32).astype(np.float64)
    L = np.asarray(lat32, np.float32).astype(np.float64).reshape(3, 3)
    S = SHIFTS.astype(np.float64)
    u = (x[None, :, None, :] - x[:n, None, None, :]) + S[None, None, :, :]
    c = [(u[..., 0] * L[0, k] + u[..., 1] * L[1, k]) + u[..., 2] * L[2, k] for k in range(3)]
    return np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])


def shortest_image_masks(frac32, lat32, n, tie_tol):
    """int32 [n][Ns]: bit s set when image s is within tie_tol of the nearest.  Asserts that no decision lies within TIE_GUARD of tie_tol."""
    d = image_dists(frac32, lat32, n)
    lim = d.min(axis=2, keepdims=True) + tie_tol
    assert not (np.abs(d - lim) < TIE_GUARD).any(), "a tie decision within 1e-9 A of tie_tol"
    bits = (d <= lim).astype(np.int64) << np.arange(IMAGES, dtype=np.int64)
    return bits.sum(axis=2).astype(np.int32)


def force_constants(Gc, mass_home, frac32, lat32, reps, h, tie_tol=TIE_TOL, det_min=1e-3):
    """(status, Phi [3 n][3 Ns], masks [n][Ns], asym) from Gc [6 n][3 Ns]; Ns from the coordinates."""
    Ns = np.asarray(frac32).reshape(-1, 3).shape[0]
    N = int(reps[0] * reps[1] * reps[2])
    if Ns < 1 or Ns > V.MAX_ATOMS or Ns % N or Ns // N > MAX_PRIM:
        return BAD_INPUT, None, None, np.nan
    n = Ns // N
    Gc = np.asarray(Gc, np.float64).reshape(6 * n, 3 * Ns)
    mass = np.asarray(mass_home, np.float64)[:n]
    if not (lattice_ok(lat32, det_min) and np.isfinite(Gc).all() and np.isfinite(mass).all() and (mass > 0).all()):
        return BAD_INPUT, np.full((3 * n, 3 * Ns), np.nan), np.zeros((n, Ns), np.int32), np.nan
    Phi = (Gc[0::2] - Gc[1::2]) / (2.0 * h)
    neg = neg_images(reps)
    P5 = Phi.reshape(n, 3, N, n, 3)
    Pp = P5[:, :, neg, :, :].transpose(3, 4, 2, 0, 1).reshape(3 * n, 3 * Ns)   # Phi'[i d; I j e] = Phi[j e; -I i d]
    mh, md = np.abs(Phi).max(), np.abs(Phi - Pp).max()
    asym = md / mh if mh > 0.0 else 0.0
    Phi = (Phi + Pp) * 0.5
    P4 = Phi.reshape(n, 3, Ns, 3)
    for i in range(n):
        s = np.zeros((3, 3))
        for at in range(Ns):
            if at != i:
                s = s + P4[i, :, at, :]
        blk = -s
        P4[i, :, i, :] = (blk + blk.T) * 0.5
    return OK, Phi, shortest_image_masks(frac32, lat32, n, tie_tol), asym


# ---- step 3: the dynamical matrix ---------------------------------------------------------------------------------------------------------------

def table_at(reps, d, r):
    base = 0 if d == 0 else (3 * reps[0] if d == 1 else 3 * (reps[0] + reps[1]))
    return 2 * (base + r + reps[d])


def phases(masks, n, reps, tab):
    """(pr, pi) [n][N][n]: (1 / mult) sum over the mask's images, ascending, of (t_a t_b) t_c."""
    N = int(reps[0] * reps[1] * reps[2])
    m3 = np.asarray(masks, np.int64).reshape(n, N, n)
    pr, pi = np.zeros((n, N, n)), np.zeros((n, N, n))
    for I, (Ia, Ib, Ic) in enumerate(images(reps)):
        for s, (Sa, Sb, Sc) in enumerate(SHIFTS):
            ta, tb, tc = (tab[k:k + 2] for k in (table_at(reps, 0, Ia + Sa * reps[0]), table_at(reps, 1, Ib + Sb * reps[1]), table_at(reps, 2, Ic + Sc * reps[2])))
            ur, ui = ta[0] * tb[0] - ta[1] * tb[1], ta[0] * tb[1] + ta[1] * tb[0]
            zr, zi = ur * tc[0] - ui * tc[1], ur * tc[1] + ui * tc[0]
            bit = ((m3[:, I, :] >> s) & 1).astype(bool)
            pr[:, I, :] = pr[:, I, :] + np.where(bit, zr, 0.0)
            pi[:, I, :] = pi[:, I, :] + np.where(bit, zi, 0.0)
    mult = np.zeros((n, N, n))
    for s in range(IMAGES):
        mult += (m3 >> s) & 1
    with np.errstate(invalid="ignore", divide="ignore"):
        return pr / mult, pi / mult


def dynmat(Phi, masks, mass_home, reps, tab, stages=None):
    """(E [6 n][6 n], herm): the real symmetric embedding of the Hermitian part of D(q)."""
    N = int(reps[0] * reps[1] * reps[2])
    n = Phi.shape[0] // 3
    mass = np.asarray(mass_home, np.float64)[:n]
    pr, pi = phases(masks, n, reps, np.asarray(tab, np.float64))
    P5 = Phi.reshape(n, 3, N, n, 3)
    sr, si = np.zeros((n, 3, n, 3)), np.zeros((n, 3, n, 3))
    for I in range(N):
        sr = sr + P5[:, :, I, :, :] * pr[:, I, :][:, None, :, None]
        si = si + P5[:, :, I, :, :] * pi[:, I, :][:, None, :, None]
    mm = np.sqrt(mass[:, None] * mass[None, :])[:, None, :, None]
    A, B = (sr / mm).reshape(3 * n, 3 * n), (si / mm).reshape(3 * n, 3 * n)
    mh = max(np.abs(A).max(), np.abs(B).max())
    md = max(np.abs(A - A.T).max(), np.abs(B + B.T).max())
    herm = md / mh if mh > 0.0 else 0.0
    if stages is not None:
        stages["A"], stages["B"] = A.copy(), B.copy()
    A, B = (A + A.T) * 0.5, (B - B.T) * 0.5
    return np.block([[A, -B], [B, A]]), herm


# ---- step 5: thermodynamics -------------------------------------------------------------------------------------------------------------------

def thermo(evals, eig_status, sweeps, herm_item, fc_status, weights, temps, nu_cut):
    """One crystal: evals [Q][6 n] ascending per item, the items in the order of their q."""
    Q, K = len(evals), len(temps)
    m = len(evals[0]) // 2 if Q else 0
    st = fc_status if fc_status != OK else max([OK] + [int(s) for s in eig_status])
    if st != OK or Q == 0:
        return dict(lam=np.full((Q, m), np.nan), freqs=np.full((Q, m), np.nan), c_v=np.full(K, np.nan), zpe=np.nan, n_imag=-1, n_zero=-1, min_freq=np.nan, min_q=-1,
                    herm=np.nan, pair_gap=np.nan, sweeps_max=-1, status=st if st != OK else BAD_INPUT)
    ev = np.asarray(evals, np.float64).reshape(Q, 2 * m)
    lam = (ev[:, 0::2] + ev[:, 1::2]) * 0.5
    top = np.abs(ev).max() if ev.size else 0.0
    gap = (ev[:, 1::2] - ev[:, 0::2]).max() if ev.size else 0.0
    gap = max(gap, 0.0)
    cs, z, wsum, ni, nz = np.zeros(K), 0.0, 0.0, 0, 0
    for q in range(Q):
        th = V.thermo(lam[q], OK, temps, nu_cut)
        w = float(weights[q])
        cs = cs + w * th["c_v"]
        z = z + w * th["zpe"]
        wsum = wsum + w
        ni, nz = ni + int(weights[q]) * th["n_imag"], nz + int(weights[q]) * th["n_zero"]
    freqs = V.frequencies(lam)
    lo, at = np.nan, -1
    for q in range(Q):
        for k in range(m):
            if at < 0 or freqs[q, k] < lo:
                lo, at = freqs[q, k], q
    return dict(lam=lam, freqs=freqs, c_v=cs / wsum, zpe=z / wsum, n_imag=ni, n_zero=nz, min_freq=lo, min_q=at, herm=max([0.0] + [float(h) for h in herm_item]),
                pair_gap=gap / top if top > 0.0 else 0.0, sweeps_max=max([0] + [int(s) for s in sweeps]), status=OK)


def analyze(model, Gc, qpoints, weights, temps=(300.0,), nu_cut=0.05, h=0.01, tie_tol=TIE_TOL, det_min=1e-3, reps=None):
    """Steps 2 to 5 of one synthetic crystal from its rows Gc."""
    reps = tuple(model["reps"]) if reps is None else tuple(reps)
    Ns = model["Ns"]
    N = reps[0] * reps[1] * reps[2]
    st, Phi, masks, asym = force_constants(Gc, model["mass"], model["frac"], model["lat"], reps, h, tie_tol, det_min)
    tab = phase_table(qpoints, reps)
    Q = len(tab)
    n = Ns // N if Ns % N == 0 else 0
    E, herm, evals, sweeps, est = [], [], [], [], []
    for q in range(Q):
        if st == OK:
            e, hm = dynmat(Phi, masks, model["mass"], reps, tab[q])
        else:   # a matrix of NaN: the solver answers BAD_INPUT (an empty one: OK, and the crystal's status says it)
            e, hm = np.full((6 * n, 6 * n), np.nan), np.nan
        lam, sw, es = V.jacobi(e)
        E.append(e), herm.append(hm), evals.append(lam), sweeps.append(sw), est.append(es)
    th = thermo(evals, est, sweeps, herm, st, weights, temps, nu_cut)
    return dict(Phi=Phi, masks=masks, asym=asym, fc_status=st, E=E, herm_item=np.asarray(herm), evals=evals, sweeps=sweeps, eig_status=est, **th)


# ---- the synthetic harmonic crystal -----------------------------------------------------------------------------------------------------------

def make_model(n, reps, seed, density=0.6, cell=4.0, lat_p=None, frac_p=None, mass=None, blocks=None):
    """A primitive cell of n atoms replicated reps times, DEFINED BY ITS FORCE CONSTANTS: symmetric positive definite 3 x 3 blocks K on a
    random set of neighbours (i, I, j) != (i, 0, i) of the given density, closed under the index symmetry (i, I, j) <-> (j, -I, i);
    Phi(0 i; I j) = -K, and the self block is the sum of the atom's K (the acoustic sum rule).  density = 1 couples every pair of the
    supercell: the model's range then exceeds half the supercell and the wrap-around images tie wherever an axis is doubled.  blocks:
    {(i, (Ia, Ib, Ic), j): K [3][3]} in place of the random set (closed under the symmetry by this function).  Masses from MODEL_MASSES."""
    rng = np.random.default_rng(seed)
    reps = tuple(int(r) for r in reps)
    N = reps[0] * reps[1] * reps[2]
    Ns = n * N
    f = rng.random((n, 3)) if frac_p is None else np.asarray(frac_p, np.float64)
    Lp = (np.eye(3) * rng.uniform(0.8 * cell, 1.2 * cell, 3)[:, None] + 0.3 * rng.uniform(-1, 1, (3, 3))) if lat_p is None else np.asarray(lat_p, np.float64)
    img, neg = images(reps), neg_images(reps)
    frac = ((f[None, :, :] + img[:, None, :]) / np.asarray(reps, np.float64)).reshape(-1, 3).astype(np.float32)
    lat = (Lp * np.asarray(reps, np.float64)[:, None]).astype(np.float32)
    m = rng.choice(MODEL_MASSES, n) if mass is None else np.asarray(mass, np.float64)
    P5 = np.zeros((n, 3, N, n, 3))
    if blocks is not None:
        todo = [(i, int(image_index(I, reps)), j, np.asarray(K, np.float64)) for (i, I, j), K in blocks.items()]
    else:
        todo = []
        for i in range(n):
            for I in range(N):
                for j in range(n):
                    if (I, j) == (0, i) or (j, int(neg[I]), i) < (i, I, j) or rng.random() >= density:
                        continue
                    a = rng.uniform(-1, 1, (3, 3))
                    todo.append((i, I, j, a @ a.T + np.eye(3) * rng.uniform(0.2, 2.0)))
    for i, I, j, K in todo:
        P5[i, :, I, j, :] = -K
        P5[j, :, neg[I], i, :] = -K.T
    for i in range(n):
        P5[i, :, 0, i, :] = 0.0
        P5[i, :, 0, i, :] = -P5[i].reshape(3, Ns, 3).sum(axis=1)
    return dict(n=n, reps=reps, N=N, Ns=Ns, f=f, lat_p=Lp, frac=frac, lat=lat, mass=m, mass_all=np.tile(m, N), Phi_true=P5.reshape(3 * n, 3 * Ns))


def model_gc(model, h, seed=0):
    """Gc [6 n][3 Ns] = float64(float32(g0 +- h Phi row)): g0 an arbitrary offset per displaced degree of freedom, which must cancel."""
    n, Ns = model["n"], model["Ns"]
    g0 = np.random.default_rng(seed).uniform(-0.5, 0.5, (3 * n, 3 * Ns))
    Gc = np.empty((6 * n, 3 * Ns))
    Gc[0::2] = (g0 + h * model["Phi_true"]).astype(np.float32)
    Gc[1::2] = (g0 - h * model["Phi_true"]).astype(np.float32)
    return Gc


def supercell_dynmat(Phi, mass_home, reps):
    """The full mass-weighted Hessian [3 Ns][3 Ns] of the supercell that the force constants Phi [3 n][3 Ns] span by translation:
    H[(J, i, d)][(J', j, e)] = Phi(0 i d; J' - J, j e)."""
    N = int(reps[0] * reps[1] * reps[2])
    n = Phi.shape[0] // 3
    img = images(reps)
    P5 = Phi.reshape(n, 3, N, n, 3)
    H = np.zeros((N, n, 3, N, n, 3))
    for J in range(N):
        diff = image_index(img - img[J], reps)     # [J'] -> the index of J' - J
        H[J] = P5[:, :, diff, :, :]
    m = np.repeat(np.tile(np.asarray(mass_home, np.float64)[:n], N), 3)
    return H.reshape(3 * n * N, 3 * n * N) / np.sqrt(m[:, None] * m[None, :])


# ---- the case file of scripts/phonon_host_check.cpp -------------------------------------------------------------------------------------------

def write_case(path, models, gcs, reps_list, tab_list, weights_list, h, tie_tol, det_min, nu_cut, temps):
    """int32 B, K; double h, tie_tol, det_min, nu_cut, temps[8]; per crystal: int32 Ns, reps[3], Q; float frac[Ns][3], lat[9]; double
    mass[n or Ns / 1]; double Gc[6 n][3 Ns] (n = Ns / N when reps divides, else nothing); double table[Q][6 (a + b + c)]; int32 weights[Q]."""
    t = np.zeros(V.MAX_TEMPS)
    t[:len(temps)] = temps
    with open(path, "wb") as f:
        f.write(np.array([len(models), len(temps)], np.int32).tobytes())
        f.write(np.array([h, tie_tol, det_min, nu_cut], np.float64).tobytes() + t.tobytes())
        for md, Gc, reps, tab, w in zip(models, gcs, reps_list, tab_list, weights_list):
            f.write(np.array([md["Ns"], reps[0], reps[1], reps[2], len(w)], np.int32).tobytes())
            f.write(np.asarray(md["frac"], np.float32).tobytes() + np.asarray(md["lat"], np.float32).tobytes())
            f.write(np.asarray(md["mass_all"], np.float64).tobytes())
            f.write(np.asarray(Gc, np.float64).tobytes())
            f.write(np.asarray(tab, np.float64).tobytes() + np.asarray(w, np.int32).tobytes())


def read_out(path, shapes, K):
    """shapes: [(n, Ns, Q)] (n = 0: reps does not divide)."""
    buf, at, out = open(path, "rb").read(), 0, []

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(buf, dtype, count, at)
        at += a.nbytes
        return a

    for n, Ns, Q in shapes:
        r = dict(fc_status=int(take(np.int32, 1)[0]), asym=float(take(np.float64, 1)[0]), Phi=take(np.float64, 9 * n * Ns).reshape(3 * n, 3 * Ns),
                 masks=take(np.int32, n * Ns).reshape(n, Ns))
        r["E"] = [None] * Q
        r["evals"], r["sweeps"], r["eig_status"], herm = [None] * Q, [0] * Q, [0] * Q, np.zeros(Q)
        for q in range(Q):
            r["E"][q] = take(np.float64, 36 * n * n).reshape(6 * n, 6 * n)
            herm[q] = take(np.float64, 1)[0]
            r["evals"][q] = take(np.float64, 6 * n)
            r["sweeps"][q], r["eig_status"][q] = (int(v) for v in take(np.int32, 2))
        r["herm_item"] = herm
        r["lam"], r["freqs"] = take(np.float64, Q * 3 * n).reshape(Q, 3 * n), take(np.float64, Q * 3 * n).reshape(Q, 3 * n)
        r["c_v"] = take(np.float64, K)
        r["zpe"], r["min_freq"], r["herm"], r["pair_gap"] = (float(v) for v in take(np.float64, 4))
        r["n_imag"], r["n_zero"], r["min_q"], r["sweeps_max"], r["status"] = (int(v) for v in take(np.int32, 5))
        out.append(r)
    assert at == len(buf)
    return out
