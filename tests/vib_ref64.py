"""A numpy float64 restatement of the Gamma-point vibration kernels (include/matinvent_hip_vib.h, matinvent_amd/csrc/vib_dynmat.h and
sym_jacobi.h), operation for operation in the headers' order -- every product and every sum rounded separately, every sum a
serial loop in ascending index order -- so that the device can be held to it bit for bit; and a synthetic periodic harmonic energy with
an analytic gradient and Hessian to feed it.  Plain numpy, no GPU."""
import numpy as np

OK, NO_CONVERGENCE, BAD_INPUT = 0, 1, 2
MAX_ATOMS, MAX_TEMPS, MAX_SWEEPS, LDS_MAX_M, MAX_M = 256, 8, 30, 128, 768
EPS = 2.0 ** -52
THZ = 15.633304
H_EV_THZ = 4.135667696923859e-3
H_KB_THZ = 47.992430733662204
X_MAX = 700.0
KB_J_MOL = 8.31446261815324        # k_B N_A, J / (K mol)
AMU_G_MOL = 1.0                    # a cell's mass in amu is its molar mass in g / mol
SPRING_MASSES = (1.008, 15.999, 55.845, 207.2)


# ---- steps 1 and 2: displacements and Cartesian gradients -----------------------------------------------------------------------------------

def mod1_f32(x):
    x = np.asarray(x, np.float32)
    r = (x - np.trunc(x)).astype(np.float32)
    return np.where(r < 0, (r + np.float32(1.0)).astype(np.float32), r).astype(np.float32)


def lattice_inverse(lat32, det_min):
    """(ok, L^-1 [9] float64) of a float32 lattice [3][3], by relax_fire.h's cofactors in float64."""
    lat32 = np.asarray(lat32, np.float32).reshape(9)
    if not np.isfinite(lat32).all():
        return False, None
    L = lat32.astype(np.float64)
    c0, c1, c2 = L[4] * L[8] - L[5] * L[7], L[5] * L[6] - L[3] * L[8], L[3] * L[7] - L[4] * L[6]
    det = (L[0] * c0 + L[1] * c1) + L[2] * c2
    if not abs(det) >= det_min:
        return False, None
    Li = np.array([L[4] * L[8] - L[5] * L[7], L[2] * L[7] - L[1] * L[8], L[1] * L[5] - L[2] * L[4],
                   L[5] * L[6] - L[3] * L[8], L[0] * L[8] - L[2] * L[6], L[2] * L[3] - L[0] * L[5],
                   L[3] * L[7] - L[4] * L[6], L[1] * L[6] - L[0] * L[7], L[0] * L[4] - L[1] * L[3]]) / det
    return True, Li


def displace(frac32, lat32, c, h, det_min=1e-3):
    """Copy c = 6 i + 2 d + s of a crystal's float32 coordinates [n][3]."""
    out = np.array(frac32, np.float32, copy=True)
    ok, Li = lattice_inverse(lat32, det_min)
    if not ok:
        return out
    i, d, s = c // 6, (c % 6) // 2, c & 1
    hs = -h if s else h
    out[i] = mod1_f32((out[i].astype(np.float64) + hs * Li[3 * d:3 * d + 3]).astype(np.float32))
    return out


def cart_grad(g32, lat32, scale, per_atom, det_min=1e-3):
    """One row of Gc [3 n] from a copy's float32 gradient [n][3] and lattice."""
    g = np.asarray(g32, np.float32).astype(np.float64)
    n = g.shape[0]
    ok, Li = lattice_inverse(lat32, det_min)
    if not ok:
        return np.full(3 * n, np.nan)
    s = scale * float(n) if per_atom else scale
    Li = Li.reshape(3, 3)
    out = np.empty((n, 3))
    for k in range(3):
        out[:, k] = s * ((g[:, 0] * Li[k, 0] + g[:, 1] * Li[k, 1]) + g[:, 2] * Li[k, 2])
    return out.reshape(-1)


# ---- step 3: the dynamical matrix -------------------------------------------------------------------------------------------------------------

def householder(mass):
    n = len(mass)
    N3 = 3 * n
    mtot = 0.0
    for j in range(n):
        mtot += mass[j]
    rt = np.sqrt(mtot)
    U = np.zeros((3, N3))
    for d in range(3):
        U[d, d::3] = np.sqrt(mass) / rt
    v = np.zeros((3, N3))
    for k in range(3):
        x = U[k]
        nn = 0.0
        for a in range(k, N3):
            nn += x[a] * x[a]
        alpha = -np.sqrt(nn) if x[k] > 0.0 else np.sqrt(nn)
        v[k, k:] = x[k:]
        v[k, k] = v[k, k] - alpha
        vn = 0.0
        for a in range(k, N3):
            vn += v[k, a] * v[k, a]
        v[k, k:] = v[k, k:] / np.sqrt(vn)
        for c in range(k + 1, 3):
            dot = 0.0
            for a in range(k, N3):
                dot += v[k, a] * U[c, a]
            U[c, k:] = U[c, k:] - (2.0 * dot) * v[k, k:]
    return v


def dynmat(Gc, mass, h, stages=None):
    """(status, R [M][M], asym) from Gc [6 n][3 n] and the masses [n]; stages (a dict) collects H, the symmetrised and sum-ruled H, D."""
    mass = np.asarray(mass, np.float64)
    n = len(mass)
    N3, M = 3 * n, 3 * n - 3
    Gc = np.asarray(Gc, np.float64).reshape(6 * n, N3)
    if not (np.isfinite(Gc).all() and np.isfinite(mass).all() and (mass > 0).all()):
        return BAD_INPUT, np.full((M, M), np.nan), np.nan
    W = (Gc[0::2] - Gc[1::2]) / (2.0 * h)
    mh, md = np.abs(W).max(), np.abs(W - W.T).max()
    asym = md / mh if mh > 0.0 else 0.0
    if stages is not None:
        stages["H"] = W.copy()
    W = (W + W.T) * 0.5
    blocks = W.reshape(n, 3, n, 3)
    for i in range(n):
        s = np.zeros((3, 3))
        for j in range(n):
            if j != i:
                s = s + blocks[i, :, j, :]
        blk = -s
        blocks[i, :, i, :] = (blk + blk.T) * 0.5
    if stages is not None:
        stages["H_asr"] = W.copy()
    mrow = np.repeat(mass, 3)
    W = W / np.sqrt(mrow[:, None] * mrow[None, :])
    if stages is not None:
        stages["D"] = W.copy()
    if M == 0:
        return OK, np.zeros((0, 0)), asym
    v = householder(mass)
    for k in range(3):
        w = np.zeros(N3)
        for b in range(N3):
            w = w + W[:, b] * v[k, b]
        K = 0.0
        for a in range(N3):
            K += v[k, a] * w[a]
        va, wa = v[k][:, None], w[:, None]
        W = ((W - (2.0 * va) * w[None, :]) - (2.0 * wa) * v[k][None, :]) + ((4.0 * K) * va) * v[k][None, :]
    if stages is not None:
        stages["QDQ"] = W.copy()
    T = W[3:, 3:]
    return OK, (T + T.T) * 0.5, asym


# ---- step 4: cyclic Jacobi, round-robin ordering ----------------------------------------------------------------------------------------------

def pairs(Me, r):
    m = Me - 1
    k = np.arange(1, Me // 2)
    a = np.concatenate([[m], (r + k) % m])
    b = np.concatenate([[r], (r - k + m) % m])
    return np.minimum(a, b), np.maximum(a, b)


def jacobi(A):
    """(eigenvalues ascending, sweeps, status) of a symmetric matrix [M][M]."""
    A = np.array(A, np.float64, copy=True)
    M = A.shape[0]
    if not np.isfinite(A).all():
        return np.full(M, np.nan), 0, BAD_INPUT
    Me = M + (M & 1)
    done, status = 0, NO_CONVERGENCE
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for _ in range(MAX_SWEEPS):
            any_sweep = False
            for r in range(Me - 1):
                p, q = pairs(Me, r)
                keep = q < M
                p, q = p[keep], q[keep]
                app, aqq, apq = A[p, p], A[q, q], A[p, q]
                rot = (apq != 0.0) & (np.abs(apq) > EPS * (np.sqrt(np.abs(app)) * np.sqrt(np.abs(aqq))))
                if not rot.any():
                    continue
                any_sweep = True
                p, q, app, aqq, apq = p[rot], q[rot], app[rot], aqq[rot], apq[rot]
                theta = (aqq - app) / (2.0 * apq)
                t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                x, y = A[:, p].copy(), A[:, q].copy()
                A[:, p] = c * x - s * y
                A[:, q] = s * x + c * y
                x, y = A[p, :].copy(), A[q, :].copy()
                A[p, :] = c[:, None] * x - s[:, None] * y
                A[q, :] = s[:, None] * x + c[:, None] * y
                A[p, p], A[q, q] = app - t * apq, aqq + t * apq
                A[p, q] = A[q, p] = 0.0
            if not any_sweep:
                status = OK
                break
            done += 1
    d = np.diag(A).copy()
    return d[np.argsort(d, kind="stable")], done, status


# ---- step 5: thermodynamics -------------------------------------------------------------------------------------------------------------------

def frequencies(lam):
    lam = np.asarray(lam, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(lam < 0.0, -(np.sqrt(np.abs(lam)) * THZ), np.sqrt(np.abs(lam)) * THZ)


def thermo(lam, status, temps, nu_cut):
    """dict(freqs, c_v [K], zpe, n_imag, n_zero, status) of one crystal's ascending eigenvalues."""
    lam = np.asarray(lam, np.float64)
    K = len(temps)
    if status != OK:
        return dict(freqs=np.full(len(lam), np.nan), c_v=np.full(K, np.nan), zpe=np.nan, n_imag=-1, n_zero=-1, status=status)
    nu = frequencies(lam)
    imag, zero = nu < -nu_cut, np.abs(nu) <= nu_cut
    live = nu[~imag & ~zero]
    c_v = np.zeros(K)
    for k, T in enumerate(temps):
        s = 0.0
        for f in live:
            x = (f * H_KB_THZ) / T
            if x < X_MAX:
                s += (x / np.expm1(x)) * (x / -np.expm1(-x))
        c_v[k] = s
    z = 0.0
    for f in live:
        z += f * H_EV_THZ
    return dict(freqs=nu, c_v=c_v, zpe=0.5 * z, n_imag=int(imag.sum()), n_zero=int(zero.sum()), status=OK)


def molar(c_v, mass_cell):
    """(J / K / mol of cells, J / K / g) from c_v in k_B and the cell's mass in amu."""
    c_mol = np.asarray(c_v, np.float64) * KB_J_MOL
    return c_mol, c_mol / mass_cell


# ---- the synthetic energy -----------------------------------------------------------------------------------------------------------------------

def make_springs(n, seed, cell=6.0, isotropic=False):
    """A crystal of n atoms in a cell with edges near `cell`, every pair joined by a spring
         E = 1/2 sum_{i < j} v_ij^T K_ij v_ij,   v_ij = w(x_j - x_i - tau_ij) L,   w(u) = u - round(u),
    with symmetric positive definite K_ij (isotropic: a multiple of the identity -> every level of the spectrum three-fold) and rest
    offsets tau_ij = tau_j - tau_i + a stretch, so that the springs are neither at rest nor near the wrap of w at 1/2 (the range condition:
    |w| < 1/4 at the start, a displacement of h / |L| << 1/4 away).  Masses from SPRING_MASSES."""
    rng = np.random.default_rng(seed)
    tau = rng.random((n, 3))
    frac = ((tau + 0.03 * rng.uniform(-1, 1, (n, 3))) % 1.0).astype(np.float32)
    lat = (np.eye(3) * rng.uniform(0.8 * cell, 1.2 * cell, 3)[:, None] + 0.3 * rng.uniform(-1, 1, (3, 3))).astype(np.float32)
    K = np.zeros((n, n, 3, 3))
    for i in range(n):
        for j in range(i + 1, n):
            if isotropic:
                Kij = np.eye(3) * rng.uniform(0.5, 5.0)
            else:
                a = rng.uniform(-1, 1, (3, 3))
                Kij = a @ a.T + np.eye(3) * rng.uniform(0.2, 2.0)
            K[i, j] = K[j, i] = Kij
    mass = rng.choice(SPRING_MASSES, n)
    return dict(n=n, tau=tau, frac=frac, lat=lat, K=K, mass=mass)


def spring_gradient(sp, frac, lat):
    """(E, g_frac [n][3]) in float64 at coordinates `frac` (any precision, read as float64) and lattice `lat`."""
    n = sp["n"]
    x, L = np.asarray(frac, np.float64), np.asarray(lat, np.float64).reshape(3, 3)
    u = (x[None, :, :] - x[:, None, :]) - (sp["tau"][None, :, :] - sp["tau"][:, None, :])   # [i][j] = (x_j - x_i) - (tau_j - tau_i)
    w = u - np.round(u)
    v = w @ L                                                                              # [i][j][3]
    Kv = np.einsum("ijab,ijb->ija", sp["K"], v)
    E = 0.25 * np.einsum("ija,ija->", v, Kv)
    g_cart = Kv.sum(axis=0)                                                                # on atom j: sum_i K_ij v_ij
    return E, g_cart @ L.T if n else np.zeros((0, 3))


def spring_hessian(sp):
    """The analytic Cartesian Hessian [3 n][3 n]."""
    n = sp["n"]
    H = np.zeros((n, 3, n, 3))
    for i in range(n):
        for j in range(n):
            if i != j:
                H[i, :, j, :] = -sp["K"][i, j]
                H[i, :, i, :] += sp["K"][i, j]
    return H.reshape(3 * n, 3 * n)


def spring_copies(sp, h, frac_of_copy=None):
    """The float32 gradients [6 n][n][3] of the displaced copies: the float64 analytic gradient at each copy's float32 coordinates (from
    `displace`, or frac_of_copy [6 n][n][3] -- the device's), rounded."""
    n = sp["n"]
    out = np.empty((6 * n, n, 3), np.float32)
    for c in range(6 * n):
        x = displace(sp["frac"], sp["lat"], c, h) if frac_of_copy is None else frac_of_copy[c]
        out[c] = spring_gradient(sp, x, sp["lat"])[1].astype(np.float32)
    return out


def analyze(sp, h, scale=1.0, per_atom=False, temps=(300.0,), nu_cut=0.05, g_copies=None):
    """Steps 2 to 5 of one synthetic crystal from its copies' float32 gradients."""
    n = sp["n"]
    g = spring_copies(sp, h) if g_copies is None else g_copies
    Gc = np.stack([cart_grad(g[c], sp["lat"], scale, per_atom) for c in range(6 * n)]) if n else np.zeros((0, 0))
    st, R, asym = dynmat(Gc, sp["mass"], h)
    lam, sweeps, est = jacobi(R) if st == OK else (np.full(3 * n - 3, np.nan), 0, BAD_INPUT)
    th = thermo(lam, est, temps, nu_cut)
    return dict(Gc=Gc, R=R, asym=asym, evals=lam, sweeps=sweeps, **th)


# ---- the host module's chunk plan (vibrations.chunk_plan restated) ----------------------------------------------------------------------------

def chunk_plan(num_atoms, batch_size):
    """[(source crystal, copy)] in order, cut into chunks of batch_size."""
    flat = [(b, c) for b, n in enumerate(num_atoms) for c in range(6 * n)]
    return [flat[s:s + batch_size] for s in range(0, len(flat), batch_size)]


# ---- the case file of scripts/vib_host_check.cpp --------------------------------------------------------------------------------------------

def write_case(path, crystals, g_copies, h, scale, per_atom, det_min, nu_cut, temps):
    t = np.zeros(MAX_TEMPS)
    t[:len(temps)] = temps
    with open(path, "wb") as f:
        f.write(np.array([len(crystals), int(per_atom), len(temps)], np.int32).tobytes())
        f.write(np.array([h, scale, det_min, nu_cut], np.float64).tobytes() + t.tobytes())
        for sp, g in zip(crystals, g_copies):
            f.write(np.array([sp["n"]], np.int32).tobytes())
            f.write(np.asarray(sp["frac"], np.float32).tobytes() + np.asarray(sp["lat"], np.float32).tobytes())
            f.write(np.asarray(g, np.float32).tobytes() + np.asarray(sp["mass"], np.float64).tobytes())


def read_out(path, num_atoms, K):
    buf, at, out = open(path, "rb").read(), 0, []

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(buf, dtype, count, at)
        at += a.nbytes
        return a

    for n in num_atoms:
        N3, M = 3 * n, 3 * n - 3
        r = dict(displaced=take(np.float32, 6 * n * N3).reshape(6 * n, n, 3), Gc=take(np.float64, 6 * n * N3).reshape(6 * n, N3),
                 dyn_status=int(take(np.int32, 1)[0]), asym=float(take(np.float64, 1)[0]), R=take(np.float64, M * M).reshape(M, M),
                 evals=take(np.float64, M), sweeps=int(take(np.int32, 1)[0]), eig_status=int(take(np.int32, 1)[0]), freqs=take(np.float64, M),
                 c_v=take(np.float64, K), zpe=float(take(np.float64, 1)[0]), n_imag=int(take(np.int32, 1)[0]), n_zero=int(take(np.int32, 1)[0]),
                 status=int(take(np.int32, 1)[0]))
        out.append(r)
    assert at == len(buf)
    return out
