"""The reference of the relaxation step (include/matinvent_hip_relax.h, matinvent_amd/csrc/relax_fire.h): `fire_step` restates one
FIRE step of a ragged batch in numpy at a chosen precision -- float64 is the reference, float32 (every operation separately rounded, the
header's order, the header's tree) is the host restatement whose own deviation from float64 scales the device's bound.  The network is
taken out: `harmonic` is a synthetic energy -- springs between every pair of atoms in fractional space with minimum-image differences,
plus a quadratic in the lattice -- whose gradients are computed in float64 from whatever state it is given.  `run` walks a batch through
consecutive steps and records, per step and crystal, the branch taken and the margin of every decision."""
import numpy as np

ACTIVE, CONVERGED, FAILED, EXHAUSTED = 0, 1, 2, 3
F_DT, F_ALPHA, F_E_FIRST, F_E_LAST, F_FMAX, F_DR, NF = 0, 1, 2, 3, 4, 5, 6
I_STATUS, I_NPOS, I_STEPS, NI = 0, 1, 2, 3
DEFAULTS = dict(dt=0.1, dt_max=1.0, maxstep=0.2, n_min=5, f_inc=1.1, f_dec=0.5, a_start=0.1, f_a=0.99, fmax=0.1, scale=1.0, cell_factor=0.0,
                det_min=1e-3, relax_cell=0, per_atom=0)
FLOATS = ("dt", "dt_max", "maxstep", "f_inc", "f_dec", "a_start", "f_a", "fmax", "scale", "cell_factor", "det_min")
# A decision counts as a tie when its float64 margin, relative to the size of its operands, is below this: float32's 6e-8 times the ~10
# roundings of a step times the 40 steps a quantity has been carried through, with an eightfold allowance for the feedback of the
# stiffest spring on top: 6e-8 x 10 x 40 x 8 = 2e-4.
TIE = 2e-4


def params(**kw):
    """The parameter set as the device receives it: every float rounded to float32 (so all precisions work on the same inputs)."""
    p = dict(DEFAULTS, **kw)
    for k in FLOATS:
        p[k] = float(np.float32(p[k]))
    return p


def tree_half(R):
    p = 1
    while p < R:
        p *= 2
    return p // 2


def tree_sum(a):
    """[G][R] -> [G]: for s = half(R), ..., 1: a[i] += a[i + s] for i < s, i + s < R."""
    a = a.copy()
    R = a.shape[1]
    s = tree_half(R)
    while s > 0:
        m = min(s, R - s)
        a[:, :m] = a[:, :m] + a[:, s:s + m]
        s //= 2
    return a[:, 0]


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def mod1(x):
    r = x - np.trunc(x)
    return np.where(r < 0, r + 1, r)


def inv3(L, dt):
    """[G][3][3] -> det [G], L^-1 [G][3][3] by cofactors, every element divided by det (the header's formulas)."""
    l = [L[:, q // 3, q % 3] for q in range(9)]
    det = (l[0] * (l[4] * l[8] - l[5] * l[7]) + l[1] * (l[5] * l[6] - l[3] * l[8])) + l[2] * (l[3] * l[7] - l[4] * l[6])
    with np.errstate(all="ignore"):
        c = [(l[4] * l[8] - l[5] * l[7]) / det, (l[2] * l[7] - l[1] * l[8]) / det, (l[1] * l[5] - l[2] * l[4]) / det,
             (l[5] * l[6] - l[3] * l[8]) / det, (l[0] * l[8] - l[2] * l[6]) / det, (l[2] * l[3] - l[0] * l[5]) / det,
             (l[3] * l[7] - l[4] * l[6]) / det, (l[1] * l[6] - l[0] * l[7]) / det, (l[0] * l[4] - l[1] * l[3]) / det]
    return det, np.stack(c, axis=1).reshape(-1, 3, 3).astype(dt)


def new_state(na, frac, lat, prm, dtype):
    B, N = len(na), int(np.sum(na))
    fs = np.zeros((B, NF), dtype)
    fs[:, F_DT], fs[:, F_ALPHA] = prm["dt"], prm["a_start"]
    return dict(frac=np.asarray(frac, dtype).reshape(N, 3).copy(), lat=np.asarray(lat, dtype).reshape(B, 3, 3).copy(), vel_x=np.zeros((N, 3), dtype),
                vel_l=np.zeros((B, 3, 3), dtype), fs=fs, is_=np.zeros((B, NI), np.int32))


def fire_step(na, prm, st, g_frac, g_lat, out_p):
    """One step of every crystal, in place on the state `st` (new_state), at the precision of its arrays.  Returns per-crystal records:
    moved, positive (F.v > 0), grew (dt grew), capped (dt_max bound the growth), clamped, and the relative margins m_P, m_fmax, m_clamp
    (inf where the decision was not taken or, P with v = 0, is exact)."""
    dt = st["frac"].dtype.type
    na = np.asarray(na)
    B = len(na)
    off = np.concatenate([[0], np.cumsum(na)])
    g_frac, g_lat, out_p = np.asarray(g_frac, dt).reshape(-1, 3), np.asarray(g_lat, dt).reshape(B, 3, 3), np.asarray(out_p, dt).reshape(B)
    rec = dict(moved=np.zeros(B, bool), positive=np.zeros(B, bool), grew=np.zeros(B, bool), capped=np.zeros(B, bool), clamped=np.zeros(B, bool),
               m_P=np.full(B, np.inf), m_fmax=np.full(B, np.inf), m_clamp=np.full(B, np.inf))
    fs, is_ = st["fs"], st["is_"]
    cell = bool(prm["relax_cell"])
    for n in np.unique(na):
        n = int(n)
        ids = np.nonzero((na == n) & (is_[:, I_STATUS] == ACTIVE))[0]
        if ids.size == 0:
            continue
        rows = (off[ids][:, None] + np.arange(n)[None]).reshape(-1)
        gx, gl, L = g_frac[rows].reshape(-1, n, 3), g_lat[ids], st["lat"][ids]
        ok = np.isfinite(out_p[ids]) & np.isfinite(gl).all(axis=(1, 2)) & np.isfinite(L).all(axis=(1, 2)) & np.isfinite(gx).all(axis=(1, 2))
        with np.errstate(all="ignore"):
            det, Li = inv3(L, dt)
            ok &= np.abs(det) >= dt(prm["det_min"])
        is_[ids[~ok], I_STATUS] = FAILED
        ids, gx, gl, L, Li = ids[ok], gx[ok], gl[ok], L[ok], Li[ok]
        if ids.size == 0:
            continue
        rows = (off[ids][:, None] + np.arange(n)[None]).reshape(-1)
        s = dt(prm["scale"]) * dt(n) if prm["per_atom"] else dt(prm["scale"])
        c = dt(prm["cell_factor"]) if prm["cell_factor"] > 0 else dt(n)
        # F[k] = -(s sum_d g[d] Li[k][d]) per atom;  -(s g_lat) / c per cell row
        F = -(s * ((gx[:, :, None, 0] * Li[:, None, :, 0] + gx[:, :, None, 1] * Li[:, None, :, 1]) + gx[:, :, None, 2] * Li[:, None, :, 2]))
        V = st["vel_x"][rows].reshape(-1, n, 3)
        if cell:
            F = np.concatenate([F, -(s * gl) / c], axis=1)
            V = np.concatenate([V, st["vel_l"][ids]], axis=1)
        ff_rows = dot3(F, F)
        fm = np.sqrt(ff_rows.max(axis=1))
        first = is_[ids, I_STEPS] == 0
        fs[ids[first], F_E_FIRST] = out_p[ids[first]]
        fs[ids, F_E_LAST], fs[ids, F_FMAX] = out_p[ids], fm
        fmax = dt(prm["fmax"])
        rec["m_fmax"][ids] = np.abs(fm.astype(np.float64) - float(fmax)) / float(fmax)
        conv = fm < fmax
        is_[ids[conv], I_STATUS] = CONVERGED
        go = ~conv
        ids, F, V, Li, L, ff_rows = ids[go], F[go], V[go], Li[go], L[go], ff_rows[go]
        if ids.size == 0:
            continue
        rows = (off[ids][:, None] + np.arange(n)[None]).reshape(-1)
        P, vv, ff = tree_sum(dot3(F, V)), tree_sum(dot3(V, V)), tree_sum(ff_rows)
        pabs = np.abs(F.astype(np.float64) * V.astype(np.float64)).sum(axis=(1, 2))
        rec["m_P"][ids] = np.where(pabs > 0, np.abs(P.astype(np.float64)) / np.where(pabs > 0, pabs, 1.0), np.inf)
        pos = P > 0
        d0, a0, np0 = fs[ids, F_DT], fs[ids, F_ALPHA], is_[ids, I_NPOS]
        with np.errstate(all="ignore"):
            c1, c2 = dt(1) - a0, a0 * (np.sqrt(vv) / np.sqrt(ff))
        grow = pos & (np0 > prm["n_min"])
        grown = d0 * dt(prm["f_inc"])
        d1 = np.where(grow, np.minimum(grown, dt(prm["dt_max"])), np.where(pos, d0, d0 * dt(prm["f_dec"])))
        a1 = np.where(grow, a0 * dt(prm["f_a"]), np.where(pos, a0, dt(prm["a_start"])))
        mixed = np.where(pos[:, None, None], c1[:, None, None] * V + np.where(pos, c2, 0)[:, None, None] * F, dt(0))
        V = (mixed + d1[:, None, None] * F).astype(dt)
        dr = d1[:, None, None] * V
        nd = np.sqrt(tree_sum(dot3(dr, dr)))
        ms = dt(prm["maxstep"])
        rec["m_clamp"][ids] = np.abs(nd.astype(np.float64) - float(ms)) / float(ms)
        clamp = nd > ms
        with np.errstate(all="ignore"):
            k = np.where(clamp, ms / nd, dt(1))
        dr = dr * k[:, None, None]
        da = dr[:, :n]
        move = (da[:, :, None, 0] * Li[:, None, 0, :] + da[:, :, None, 1] * Li[:, None, 1, :]) + da[:, :, None, 2] * Li[:, None, 2, :]
        st["frac"][rows] = mod1(st["frac"][rows].reshape(-1, n, 3) + move).reshape(-1, 3)
        st["vel_x"][rows] = V[:, :n].reshape(-1, 3)
        if cell:
            st["lat"][ids] = L + dr[:, n:] / c
            st["vel_l"][ids] = V[:, n:]
        fs[ids, F_DT], fs[ids, F_ALPHA], fs[ids, F_DR] = d1, a1, nd
        is_[ids, I_NPOS] = np.where(pos, np0 + 1, 0)
        is_[ids, I_STEPS] += 1
        rec["moved"][ids], rec["positive"][ids], rec["clamped"][ids] = True, pos, clamp
        rec["grew"][ids] = grow & (d1 > d0)
        rec["capped"][ids] = grow & (grown >= dt(prm["dt_max"]))
    return rec


# ---- the synthetic energy ---------------------------------------------------------------------------------------------------------------

def harmonic(na, spec, frac, lat):
    """Float64 energy [B] and gradients (g_frac [N][3], g_lat [B][3][3]) of
         E_b = (kx_b / (2 n_b)) sum_{i < j} |w((x_j - tau_j) - (x_i - tau_i))|^2 + (kl_b / 2) |L - L0|_F^2,   w(u) = u - round(u),
    from the state it is given (any precision; read as float64).  spec: dict(tau [N][3], L0 [B][3][3], kx [B], kl [B])."""
    na = np.asarray(na)
    B = len(na)
    off = np.concatenate([[0], np.cumsum(na)])
    x, L = np.asarray(frac, np.float64).reshape(-1, 3), np.asarray(lat, np.float64).reshape(B, 3, 3)
    d = x - spec["tau"]
    E, gx = np.zeros(B), np.zeros_like(x)
    for n in np.unique(na):
        n = int(n)
        ids = np.nonzero(na == n)[0]
        rows = (off[ids][:, None] + np.arange(n)[None]).reshape(-1)
        dd = d[rows].reshape(-1, n, 3)
        u = dd[:, None, :, :] - dd[:, :, None, :]   # [G][i][j] = d_j - d_i
        w = u - np.round(u)
        k = (spec["kx"][ids] / n)[:, None, None]
        E[ids] = 0.25 * k[:, 0, 0] * (w * w).sum(axis=(1, 2, 3))   # (every pair twice)
        gx[rows] = (k * w.sum(axis=1)).reshape(-1, 3)              # d E / d x_j = (kx / n) sum_i w_ij
    dl = L - spec["L0"]
    E += 0.5 * spec["kl"] * (dl * dl).sum(axis=(1, 2))
    return E, gx, spec["kl"][:, None, None] * dl


def make_case(na, seed, amp=0.08, lat_amp=0.3):
    """A batch and its energy: target positions tau, start positions tau + displacements up to `amp` (far from the wrap of w at 1/2),
    a target lattice L0 with the start off it by up to lat_amp; stiffnesses spread over two decades, so that the crystals of one batch take
    different branches.  A one-atom crystal starts ON its target lattice: its force is exactly zero."""
    rng = np.random.default_rng(seed)
    na = np.asarray(na)
    B, N = len(na), int(na.sum())
    tau = rng.random((N, 3))
    frac = (tau + amp * rng.uniform(-1, 1, (N, 3)) * np.repeat(rng.uniform(0.2, 1.0, B), na)[:, None]) % 1.0
    L0 = np.eye(3)[None] * rng.uniform(4.0, 7.0, (B, 3))[:, :, None] + 0.4 * rng.uniform(-1, 1, (B, 3, 3))
    lat = L0 + lat_amp * rng.uniform(-1, 1, (B, 3, 3))
    lat[na == 1] = L0[na == 1]
    spec = dict(tau=tau, L0=L0, kx=10.0 ** rng.uniform(0.5, 2.8, B), kl=10.0 ** rng.uniform(0.0, 1.5, B) * na.astype(np.float64) ** 2)
    frac32, lat32 = frac.astype(np.float32), lat.astype(np.float32)
    spec["L0"][na == 1] = lat32[na == 1].astype(np.float64)   # (exactly the float32 start)
    return dict(na=na.tolist(), spec=spec, frac=frac32, lat=lat32)


def run(case, prm, steps, dtype, step_fn=None):
    """`steps` consecutive steps from the case's start at `dtype`; the gradients come from `harmonic` at every state, rounded to dtype.
    step_fn(st, g_frac, g_lat, out) replaces fire_step (the device's form; it returns nothing).  Returns (state, the steps' records)."""
    st = new_state(case["na"], case["frac"], case["lat"], prm, dtype)
    recs = []
    for _ in range(steps):
        E, gx, gl = harmonic(case["na"], case["spec"], st["frac"], st["lat"])
        if step_fn is None:
            recs.append(fire_step(case["na"], prm, st, gx.astype(dtype), gl.astype(dtype), E.astype(dtype)))
        else:
            step_fn(st, gx.astype(dtype), gl.astype(dtype), E.astype(dtype))
    return st, recs


def branch_report(case, recs, st):
    """What the reference run took: counts per branch, the smallest margin per decision, and whether a one-atom crystal converged at step 0."""
    na = np.asarray(case["na"])
    cat = lambda k: np.stack([r[k] for r in recs])
    moved, pos = cat("moved"), cat("positive")
    nonpos_after_first = (moved & ~pos)[1:].any()
    conv_step = np.where(st["is_"][:, I_STATUS] == CONVERGED, st["is_"][:, I_STEPS], -1)
    return dict(nonpositive=bool(nonpos_after_first), grew=bool(cat("grew").any()), capped=bool(cat("capped").any()), clamped=bool(cat("clamped").any()),
                converged_mid_run=bool(((conv_step > 0) & (conv_step < len(recs) - 1)).any()),
                one_atom_at_step_0=bool((na == 1).any() and (conv_step[na == 1] == 0).all()),
                m_P=float(cat("m_P").min()), m_fmax=float(cat("m_fmax").min()), m_clamp=float(cat("m_clamp").min()))


def deviation(a, b):
    """Per array (and per column of the float block), the largest absolute difference of two states (coordinates on the circle); the int
    block must agree exactly."""
    out = {}
    for k in ("frac", "lat", "vel_x", "vel_l"):
        d = np.abs(np.asarray(a[k], np.float64) - np.asarray(b[k], np.float64))
        if k == "frac":
            d = np.minimum(d, 1.0 - d)
        out[k] = float(d.max()) if d.size else 0.0
    for j, k in enumerate(("dt", "alpha", "e_first", "e_last", "fmax", "dr")):   # the float block, column by column
        out[k] = float(np.abs(np.asarray(a["fs"][:, j], np.float64) - np.asarray(b["fs"][:, j], np.float64)).max()) if len(a["fs"]) else 0.0
    out["is_equal"] = bool(np.array_equal(a["is_"], b["is_"]))
    return out
