"""The refined structure of DESIGN 55 restated in numpy / plain Python float64, operation for operation, on top of tests/sym_ref64.py: the
executable form of the definition in include/matinvent_hip_sym_refine.h, and the reference every output of mi_sym_refine is held to bit
for bit.  Beside the entry's outputs refine() returns, per crystal, what the certificates need in float64 before any rounding: the mean
metric Gbar, the refined coordinates in the prepared basis and the site maps."""
import math

import numpy as np

from tests import sm_cases as K
from tests import sm_ref64 as R
from tests import sym_ref64 as S

REFINE_FAIL, NINFO, NSTAT = 1024, 8, 4
INFO = ("n_orbits", "n_ops", "zero2", "zero3", "zero4", "zero5", "zero6", "status")
KEYS = ("info", "stat", "orbit", "mult", "site_order", "trans_ref", "frac", "lat")


def congruence(W, G):
    """W G W^T of an integer W: (W G) first, then (W G) W^T."""
    A = [(float(W[3 * i]) * G[j] + float(W[3 * i + 1]) * G[3 + j]) + float(W[3 * i + 2]) * G[6 + j] for i in range(3) for j in range(3)]
    return [(A[3 * i] * float(W[3 * j]) + A[3 * i + 1] * float(W[3 * j + 1])) + A[3 * i + 2] * float(W[3 * j + 2]) for i in range(3) for j in range(3)]


def mean_metric(G, rot):
    Gbar = [0.0] * 9
    for W in rot:
        B = congruence([int(v) for v in W], G)
        Gbar = [Gbar[e] + B[e] for e in range(9)]
    return [g / float(len(rot)) for g in Gbar]


def refine_cell(lat32, rot):
    """(ok, T, Gbar, change, cell [9] float32) from the caller's float32 cell and the rotation parts."""
    ok, T, Lr = R.reduce_cell([float(v) for v in lat32])
    assert ok
    G = S.rigid_metric(Lr)
    Gbar = mean_metric(G, rot)
    change = max(abs(Gbar[e] - G[e]) for e in range(9)) / max(abs(g) for g in G)
    Gc = congruence(R.iadj3(T), Gbar)
    out = np.zeros(9, np.float32)
    if not Gc[0] > 0.0:
        return False, T, Gbar, change, out
    l00 = math.sqrt(Gc[0])
    l10, l20 = Gc[3] / l00, Gc[6] / l00
    p1 = Gc[4] - l10 * l10
    if not p1 > 0.0:
        return False, T, Gbar, change, out
    l11 = math.sqrt(p1)
    l21 = (Gc[7] - l20 * l10) / l11
    p2 = (Gc[8] - l20 * l20) - l21 * l21
    if not p2 > 0.0:
        return False, T, Gbar, change, out
    out[[0, 3, 4, 6, 7, 8]] = [np.float32(v) for v in (l00, l10, l11, l20, l21, math.sqrt(p2))]
    return True, T, Gbar, change, out


def min_image(G, z, x):
    """sm_pair_cost's vector of the pairs (x[i], z[i] + 0): rows [n, 3]."""
    d = (z + 0.0) - x
    D = d - np.floor(d + 0.5)
    best = np.full(len(D), R.INF)
    u = D.copy()
    for kx in (-1, 0, 1):
        for ky in (-1, 0, 1):
            for kz in (-1, 0, 1):
                a, b, c = D[:, 0] + float(kx), D[:, 1] + float(ky), D[:, 2] + float(kz)
                q = R.quad(G, a, b, c)
                better = q < best
                best = np.where(better, q, best)
                u = np.where(better[:, None], np.stack([a, b, c], axis=-1), u)
    return u


def tree64(values, op):
    v = [float(x) for x in values] + [0.0] * (64 - len(values))
    s = 32
    while s >= 1:
        for i in range(s):
            v[i] = op(v[i], v[i + s])
        s //= 2
    return v[0]


def site_maps(G, f, so, nspec, rot, trans):
    """(sigma [nops, n], residual [nops, n, 3], the largest squared residual)."""
    nops, n = len(rot), len(f)
    sig, res, d2max = np.zeros((nops, n), np.int64), np.zeros((nops, n, 3)), 0.0
    for k in range(nops):
        img = R.map_frac(f, R.map_inverse([int(v) for v in rot[k]]))
        for s in range(nspec):
            b0, b1 = so[s], so[s + 1]
            at, d2, u = S.nearest(G, f[b0:b1], img[b0:b1], np.asarray(trans[k], np.float64)[None, :])
            sig[k, b0:b1], res[k, b0:b1] = b0 + at[0], u[0]
            d2max = max(d2max, float(d2.max()))
    return sig, res, d2max


def project(G, f, sig, rot, trans, res):
    """(tbar [nops, 3], xbar [n, 3], q [n]) of steps 2 and 3."""
    nops, n = sig.shape
    tbar = np.zeros((nops, 3))
    for k in range(nops):
        s = [0.0, 0.0, 0.0]
        for i in range(n):
            s = [s[c] + float(res[k, i, c]) for c in range(3)]
        tbar[k] = [float(trans[k][c]) - s[c] / float(n) for c in range(3)]
    acc = np.zeros((n, 3))
    for k in range(nops):
        W = [float(v) for v in rot[k]]
        y = f[sig[k]] - tbar[k][None, :]
        z = np.stack([(y[:, 0] * W[c] + y[:, 1] * W[3 + c]) + y[:, 2] * W[6 + c] for c in range(3)], axis=1)
        acc = acc + min_image(G, z, f)
    m = acc / float(nops)
    q = R.quad(G, m[:, 0], m[:, 1], m[:, 2])
    return tbar, f + m, np.where(q > 0.0, q, 0.0)


def core(G, f, so, nspec, perm, rot, trans):
    """Steps 1 to 4 for one crystal in the prepared basis: dict of sigma, tbar, xbar, q, d2max, low, mult, stab and bad (a map that is no
    bijection or an orbit whose size times its site order is not n_ops)."""
    nops, n = len(rot), len(f)
    sig, res, d2max = site_maps(G, f, so, nspec, rot, trans)
    bad = any(len(set(int(v) for v in sig[k])) != n for k in range(nops))
    tbar, xbar, q = project(G, f, sig, rot, trans, res)
    low = [min(perm[int(j)] for j in sig[:, i]) for i in range(n)]
    mult = [len(set(int(j) for j in sig[:, i])) for i in range(n)]
    stab = [int((sig[:, i] == i).sum()) for i in range(n)]
    bad = bad or any(mult[i] * stab[i] != nops for i in range(n))
    return {"sigma": sig, "tbar": tbar, "xbar": xbar, "q": q, "d2max": d2max, "low": low, "mult": mult, "stab": stab, "bad": bad}


def refine(P, types, frac, lat, F, fill=0, exact=False):
    """mi_sym_refine over a prepared set P and the find arrays F: dict of info [B, 8], stat [B, 4], orbit, mult, site_order [N], trans_ref
    [B, 192, 3], frac [N, 3] float32, lat [B, 9] float32; rows the kernel does not write keep `fill`.  "extra": per crystal None or a dict of
    Gbar, rot, tbar, xbar, sigma, G, f, perm, T, so, nspec (float64, unrounded).  exact=True takes the cell in float64 as it is given (with
    a prepared set of prepare_exact); the float32 outputs are then rounded from it."""
    frac, lat = np.asarray(frac, np.float32).reshape(-1, 3), np.asarray(lat, np.float64 if exact else np.float32).reshape(-1, 9)
    B, N = len(lat), len(frac)
    out = {"info": np.full((B, NINFO), fill, np.int32), "stat": np.full((B, NSTAT), float(fill)), "orbit": np.full(N, fill, np.int32),
           "mult": np.full(N, fill, np.int32), "site_order": np.full(N, fill, np.int32), "trans_ref": np.full((B, S.MAX_OPS, 3), float(fill)),
           "frac": np.full((N, 3), fill, np.float32), "lat": np.full((B, 9), fill, np.float32), "extra": [None] * B}
    for b in range(B):
        pinfo = P["info"][b]
        st, nops = int(F["info"][b][7]), int(F["info"][b][0])
        n, nspec = int(pinfo[0]), int(pinfo[1])
        out["stat"][b] = 0.0
        if pinfo[3] != R.PREP_OK or n < 1 or n > R.MAX_ATOMS:
            out["info"][b] = [0] * (NINFO - 1) + [st | S.NOT_PREPARED | REFINE_FAIL]
            continue
        n0 = int(P["offsets"][b])

        def copy(n_ops, status):
            out["frac"][n0:n0 + n], out["lat"][b] = frac[n0:n0 + n], lat[b]
            out["orbit"][n0:n0 + n], out["mult"][n0:n0 + n], out["site_order"][n0:n0 + n] = np.arange(n), 1, 1
            out["info"][b] = [n, n_ops] + [0] * (NINFO - 3) + [status]

        if st != S.OK or nops < 1 or nops > S.MAX_OPS:
            copy(nops, st | REFINE_FAIL)
            continue
        if nops == 1:
            copy(1, st)
            continue
        f = np.array(P["frac"][n0:n0 + n], np.float64)
        so, perm = [int(v) for v in P["spec_off"][b]], [int(v) for v in P["perm"][n0:n0 + n]]
        G = S.rigid_metric([float(x) for x in P["lat"][b]])
        rot, trans = np.asarray(F["rot"][b][:nops]), np.asarray(F["trans"][b][:nops], np.float64)
        c = core(G, f, so, nspec, perm, rot, trans)
        sig, tbar, xbar, q, d2max, low, mult, stab = (c[k] for k in ("sigma", "tbar", "xbar", "q", "d2max", "low", "mult", "stab"))
        ok, T, Gbar, change, cell = refine_cell(lat[b], rot)
        bad = c["bad"] or not ok
        if bad:
            copy(nops, st | REFINE_FAIL)
            continue
        for i in range(n):
            row = []
            for c in range(3):
                w = np.float32(R.wrap01((float(xbar[i, 0]) * float(T[c]) + float(xbar[i, 1]) * float(T[3 + c])) + float(xbar[i, 2]) * float(T[6 + c])))
                row.append(np.float32(0.0) if w >= np.float32(1.0) else w)
            at = n0 + perm[i]
            out["frac"][at], out["orbit"][at], out["mult"][at], out["site_order"][at] = row, low[i], mult[i], stab[i]
        out["lat"][b], out["trans_ref"][b, :nops] = cell, tbar
        out["info"][b] = [sum(1 for i in range(n) if low[i] == perm[i]), nops] + [0] * (NINFO - 3) + [st]
        out["stat"][b] = [math.sqrt(tree64(q, max)), math.sqrt(tree64(q, lambda x, y: x + y) / float(n)), change, math.sqrt(d2max)]
        out["extra"][b] = {"Gbar": Gbar, "rot": rot, "tbar": tbar, "xbar": xbar, "sigma": sig, "G": G, "f": f, "perm": perm, "T": T, "so": so, "nspec": nspec}
    return out


def chain(batch, symprec, cos_tol, fill=0, margin=False):
    """prepare -> find -> refine of a batch (offsets, types, frac, lat): dict of P, tol, F and ref."""
    P = R.prepare(*batch)
    tol = S.tolerances(batch[0], batch[3], symprec)
    F = S.find(P, tol, cos_tol, fill=fill, margin=margin)
    return {"P": P, "tol": tol, "F": F, "ref": refine(P, batch[1], batch[2], batch[3], F, fill=fill)}


def prepare_exact(crystals):
    """(batch, P): the prepared set of float64 crystals without the float32 rounding of the interface -- the order, the blocks and perm of
    R.prepare, the cell and the coordinates from the float64 input by the same formulas.  batch[3] is the float64 cell."""
    batch = K.batch(crystals)
    P = R.prepare(*batch)
    lat64 = np.stack([np.asarray(c[0], np.float64).reshape(9) for c in crystals])
    for b, (L, z, f) in enumerate(crystals):
        assert P["info"][b][3] == R.PREP_OK
        n0, n = int(batch[0][b]), len(z)
        st, T, Ls, inv = R.prepare_cell([float(v) for v in lat64[b]], n)
        assert st == R.PREP_OK
        P["lat"][b], P["inv"][b] = Ls, inv
        A = R.iadj3(T)
        f = np.asarray(f, np.float64).reshape(-1, 3)
        for pos in range(n):
            a = int(P["perm"][n0 + pos])
            P["frac"][n0 + pos] = [R.wrap01((float(f[a, 0]) * float(A[c]) + float(f[a, 1]) * float(A[3 + c])) + float(f[a, 2]) * float(A[6 + c])) for c in range(3)]
    return (batch[0], batch[1], batch[2], lat64), P


def chain_exact(crystals, symprec, cos_tol):
    """chain() on float64 crystals as they are typed."""
    batch, P = prepare_exact(crystals)
    tol = S.tolerances(batch[0], batch[3].astype(np.float32), symprec)
    F = S.find(P, tol, cos_tol, margin=False)
    return {"P": P, "tol": tol, "F": F, "ref": refine(P, batch[1], batch[2], batch[3], F, exact=True)}


def again(extra, n):
    """The refined float64 structure refined once more with the group found: the coordinates xbar (wrapped) under the metric Gbar in the
    prepared scale, the operations (W_k, tbar_k).  Returns (the largest move in the prepared units, the largest relative change of Gbar)."""
    Gbar = extra["Gbar"]
    vol = math.sqrt(abs(R.det3(Gbar)))
    s = (float(n) / vol) ** (1.0 / 3.0)
    G2 = [g * s * s for g in Gbar]
    f2 = R.vwrap01(extra["xbar"])
    c = core(G2, f2, extra["so"], extra["nspec"], extra["perm"], extra["rot"], extra["tbar"])
    assert not c["bad"]
    G3 = mean_metric(Gbar, extra["rot"])
    return math.sqrt(float(c["q"].max())), max(abs(G3[e] - Gbar[e]) for e in range(9)) / max(abs(g) for g in Gbar)


def crystal_of(batch, ref, b):
    """Crystal b of the refined outputs as (lattice [3, 3], types, frac) in float64."""
    lo, hi = int(batch[0][b]), int(batch[0][b + 1])
    return ref["lat"][b].reshape(3, 3).astype(np.float64), [int(v) for v in batch[1][lo:hi]], ref["frac"][lo:hi].astype(np.float64)


def analyse(crystals, symprec, margin=False):
    """(n_ops, point group name, status) per crystal under the restated finder."""
    batch = K.batch(crystals)
    P = R.prepare(*batch)
    F = S.find(P, S.tolerances(batch[0], batch[3], symprec), K.COS_TOL, margin=margin)
    return [(int(r[0]), S.PG_NAMES[int(r[4]) - 1] if r[4] else "", int(r[7])) for r in F["info"]]


def partition(orbit):
    """The orbit partition as a set of frozensets of atom indices."""
    groups = {}
    for i, o in enumerate(orbit):
        groups.setdefault(int(o), set()).add(i)
    return {frozenset(g) for g in groups.values()}


def chain_cell(batch, symprec, cos_tol, cell="given", fill=0):
    """refine_arrays of matinvent_amd/symmetry.py under the restatement: dict of offsets, types, frac, lat, orbit, mult, site_order, info,
    stat (the rows of a crystal the prepare guard of the last stage rejected are that stage's input, every atom an orbit of its own)."""
    from tests import conv_ref64 as CV
    off, types, frac, lat = batch
    earlier = np.zeros(len(lat), np.int32)
    if cell == "primitive":
        P = R.prepare(*batch)
        F = S.find(P, S.tolerances(off, lat, symprec), cos_tol, margin=False)
        p = S.primitive(P, types, frac, lat, F, margin=False)
        off, types, frac, lat, earlier = p["prim_offsets"], p["types"], p["frac"], p["lat"], p["prim_status"] & S.PRIM_FAIL
    elif cell == "conventional":
        c = CV.chain(batch, symprec, cos_tol)["conv"]
        off, types, frac, lat, earlier = c["conv_offsets"], c["types"], c["frac"], c["lat"], c["conv_info"][:, 7] & CV.CONV_FAIL
    else:
        assert cell == "given"
    tol = S.tolerances(batch[0], batch[3], symprec)   # the caller's: V / n is kept
    P = R.prepare(off, types, frac, lat)
    F = S.find(P, tol, cos_tol, margin=False)
    ref = refine(P, types, frac, lat, F, fill=fill)
    out = {k: np.array(ref[k], copy=True) for k in ("frac", "lat", "orbit", "mult", "site_order", "info", "stat")}
    for b in range(len(lat)):
        if out["info"][b, 7] & S.NOT_PREPARED:
            lo, hi = int(off[b]), int(off[b + 1])
            if 0 <= lo <= hi <= len(frac):
                out["frac"][lo:hi], out["orbit"][lo:hi], out["mult"][lo:hi], out["site_order"][lo:hi] = np.asarray(frac, np.float32)[lo:hi], np.arange(hi - lo), 1, 1
            out["lat"][b] = np.asarray(lat, np.float32).reshape(-1, 9)[b]
    out["info"][:, 7] |= earlier.astype(np.int32)
    out["offsets"], out["types"] = np.asarray(off, np.int32), np.asarray(types, np.int32)
    return out


def cell_parameters(L):
    L = np.asarray(L, np.float64).reshape(3, 3)
    ln = np.linalg.norm(L, axis=1)
    cos = [float(L[i] @ L[j] / (ln[i] * ln[j])) for i, j in ((1, 2), (0, 2), (0, 1))]
    return [float(v) for v in ln] + [math.degrees(math.acos(max(-1.0, min(1.0, c)))) for c in cos]
