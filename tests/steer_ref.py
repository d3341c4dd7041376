"""Reference arithmetic of the particle resampling (include/matinvent_hip_steer.h, matinvent_amd/csrc/steer_plan.h): a float64
restatement of the plan of one group.  What the device STORES -- the scores u, the log-weights lw, and through them u_prev and logw -- is
formed by the header's own separately rounded float32 operations (numpy float32 reproduces them bit for bit); every DECISION -- the
weights, their sums, the effective sample size, the thresholds and the search -- is taken in float64 from those stored values.  A
group is `safe` when every float64 threshold lies further than margin * sum w from every cumulative boundary and the ESS lies further
than margin * K from its limit: there the fp32 plan must take the same decisions (the margin is derived in tests/test_gpu_steer.py).
Plain numpy, CPU; a helper, not a test."""
import numpy as np

from oracle import diffcsp_oracle as O

MODE_MAX, MODE_MIN, MODE_TARGET = 0, 1, 2
RESAMPLED, NO_FINITE = 1, 2
DRAW_STEER = 29
MARGIN = 1e-4
F32_MAX = np.float32(3.402823466e+38)


def score(o, mode, target=0.0):
    o = np.asarray(o, dtype=np.float32)
    if mode == MODE_MAX:
        return o.copy()
    if mode == MODE_MIN:
        return -o
    with np.errstate(invalid="ignore"):
        return -np.abs(o - np.float32(target))


def logweight(logw, lam, u, u_prev):
    """steer_logweight: float32, one rounding per operation; weight 0 (-inf) for a non-finite score or a NaN result."""
    logw, u, u_prev = (np.asarray(v, dtype=np.float32) for v in (logw, u, u_prev))
    with np.errstate(invalid="ignore", over="ignore"):
        d = u - u_prev
        s = np.float32(lam) * d
        lw = logw + s
    lw = np.where(~np.isfinite(u) | np.isnan(lw), np.float32(-np.inf), lw).astype(np.float32)
    return np.minimum(lw, F32_MAX).astype(np.float32)


def uniforms(seed, level, G, K, graph_offset=0):
    """The groups' uniforms: Philox draw 29 at step `level`, element = the global index of the group's first crystal."""
    return O.philox_uniform(int(seed), int(level), DRAW_STEER, G * K, int(graph_offset))[::K].astype(np.float32)


def plan_group(u, u_prev, logw, lam, ess_frac, U, margin=MARGIN):
    """One group -> dict(anc [K] (inside the group), u_prev, logw (float32), ess (float64), flags, safe)."""
    u, u_prev, logw = (np.asarray(v, dtype=np.float32) for v in (u, u_prev, logw))
    K = len(u)
    lw = logweight(logw, lam, u, u_prev)
    ident = np.arange(K)
    if not np.isfinite(lw).any():
        return dict(anc=ident, u_prev=u_prev.copy(), logw=logw.copy(), ess=0.0, flags=NO_FINITE, safe=True)
    l64 = lw.astype(np.float64)
    m = l64.max()
    with np.errstate(under="ignore"):
        w = np.where(np.isneginf(l64), 0.0, np.exp(l64 - m))
    S, Q = w.sum(), (w * w).sum()
    ess = S * S / Q
    limit = float(ess_frac) * K
    resample = ess_frac < 0 or ess < limit
    safe = ess_frac < 0 or abs(ess - limit) > margin * K
    if not resample:
        return dict(anc=ident, u_prev=u.copy(), logw=lw, ess=ess, flags=0, safe=safe)
    anc = ident
    if not np.all(lw == lw[0]):
        c = np.cumsum(w)
        t = (np.float64(U) + np.arange(K)) / K * S
        last = int(np.nonzero(w > 0)[0][-1])
        anc = np.minimum(np.searchsorted(c, t, side="right"), last)
        safe = safe and float(np.abs(t[:, None] - c[None, :]).min()) > margin * S
    return dict(anc=anc, u_prev=u[anc].copy(), logw=np.zeros(K, np.float32), ess=ess, flags=RESAMPLED, safe=safe)


def plan(out, p, mode, target, lam, ess_frac, K, u_prev, logw, U, margin=MARGIN):
    """A whole call: out [B][P], u_prev / logw [B], U [G] -> dict(ancestors [B] (crystal indices), u_prev, logw, stats [3] float64,
    ess [G], flags [G], safe [G])."""
    out = np.asarray(out, dtype=np.float32)
    B = out.shape[0]
    G = B // K
    u = score(out[:, p], mode, target)
    res = dict(ancestors=np.zeros(B, np.int64), u_prev=np.zeros(B, np.float32), logw=np.zeros(B, np.float32), ess=np.zeros(G), flags=np.zeros(G, np.int64),
               safe=np.zeros(G, bool))
    for g in range(G):
        s = slice(g * K, (g + 1) * K)
        r = plan_group(u[s], u_prev[s], logw[s], lam, ess_frac, U[g], margin)
        res["ancestors"][s] = g * K + r["anc"]
        res["u_prev"][s], res["logw"][s] = r["u_prev"], r["logw"]
        res["ess"][g], res["flags"][g], res["safe"][g] = r["ess"], r["flags"], r["safe"]
    res["stats"] = np.array([(res["flags"] & RESAMPLED).astype(bool).sum(), res["ess"].sum(), (res["flags"] & NO_FINITE).astype(bool).sum()], dtype=np.float64)
    return res


def gather_rows(num_atoms, ancestors):
    """Row indices of a ragged gather: the atoms of crystal ancestors[c] for every c, in order."""
    off = np.concatenate([[0], np.cumsum(num_atoms)])
    return np.concatenate([np.arange(off[a], off[a + 1]) for a in ancestors]) if len(ancestors) else np.zeros(0, np.int64)
