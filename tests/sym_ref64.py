"""The symmetry finder of DESIGN 50 restated in numpy / plain Python float64, operation for operation, on top of tests/sm_ref64.py: the
executable form of the definition, and the reference every output of mi_sym_find and mi_sym_primitive is held to bit for bit.  Also the
derivation of the 32 point groups' class histograms from generator sets (the table csrc/sym_ops.h ships is compared with it), and the
certificate: a check of returned operations from the input alone.  Every decision against the tolerance or the determinant test is
asserted to lie more than MARGIN away from it (margin=False switches the assert off for timing runs)."""
import itertools
import math
from functools import lru_cache

import numpy as np

from tests import sm_ref64 as R

MAX_OPS, MAX_TRANS, NINFO, NCLASS = 192, 64, 8, 10
OK, NOT_PREPARED, BOX_CAP, MAP_CAP, NO_LATTICE, AMBIGUOUS, OPS_CAP, NOT_A_GROUP, PRIM_FAIL, BAD_TOL = 0, 1, 2, 4, 8, 16, 32, 64, 128, 256
CLASSES = (-6, -4, -3, -2, -1, 1, 2, 3, 4, 6)
PG_NAMES = ("1", "-1", "2", "m", "2/m", "222", "mm2", "mmm", "4", "-4", "4/m", "422", "4mm", "-42m", "4/mmm", "3", "-3", "32", "3m", "-3m", "6", "-6", "6/m",
            "622", "6mm", "-6m2", "6/mmm", "23", "m-3", "432", "-43m", "m-3m")
PG_ORDERS = (1, 2, 2, 2, 4, 4, 4, 8, 4, 4, 8, 8, 8, 8, 16, 3, 6, 6, 6, 12, 6, 6, 12, 12, 12, 12, 24, 12, 24, 24, 24, 48)
IDENT = [1, 0, 0, 0, 1, 0, 0, 0, 1]
MARGIN = 1e-9
INFO = ("n_ops", "n_trans", "n_maps", "pg_order", "pg_index", "crystal_system", "has_inversion", "status")


# ---- the 32 point groups from generators -------------------------------------------------------------------------------------------------------
def rot_class(M):
    """index into CLASSES by (determinant, trace), or -1."""
    d, tr = R.idet3(M), M[0] + M[4] + M[8]
    if d == 1:
        return {3: 5, -1: 6, 0: 7, 1: 8, 2: 9}.get(tr, -1)
    if d == -1:
        return {-3: 4, 1: 3, 0: 2, -1: 1, -2: 0}.get(tr, -1)
    return -1


def close_group(gens):
    """The finite group of integer 3 x 3 matrices the generators generate, as a set of 9-tuples."""
    ident = np.eye(3, dtype=np.int64)
    group, frontier = {tuple(ident.reshape(9))}, [ident]
    gens = [np.array(g, np.int64).reshape(3, 3) for g in gens]
    while frontier:
        nxt = []
        for a in frontier:
            for g in gens:
                p = a @ g
                k = tuple(int(v) for v in p.reshape(9))
                if k not in group:
                    assert len(group) < 200
                    group.add(k)
                    nxt.append(p)
        frontier = nxt
    return group


@lru_cache(maxsize=None)
def derive_point_groups():
    """[(name, order, histogram)] of the 32 crystallographic point groups, the hexagonal family in a hexagonal basis."""
    neg = lambda M: [-v for v in M]
    inv = neg(IDENT)
    c2z, c2x = [-1, 0, 0, 0, -1, 0, 0, 0, 1], [1, 0, 0, 0, -1, 0, 0, 0, -1]
    mz, mx = [1, 0, 0, 0, 1, 0, 0, 0, -1], [-1, 0, 0, 0, 1, 0, 0, 0, 1]
    c4z, c3d = [0, -1, 0, 1, 0, 0, 0, 0, 1], [0, 0, 1, 1, 0, 0, 0, 1, 0]
    c6h = [1, -1, 0, 1, 0, 0, 0, 0, 1]                       # hexagonal basis, 60 degrees about c
    c3h = [0, -1, 0, 1, -1, 0, 0, 0, 1]
    c2a = [1, -1, 0, 0, -1, 0, 0, 0, -1]                     # a two-fold axis in the plane
    ma = neg(c2a)
    gens = {"1": [], "-1": [inv], "2": [c2z], "m": [mz], "2/m": [c2z, inv], "222": [c2z, c2x], "mm2": [c2z, mx], "mmm": [c2z, c2x, inv],
            "4": [c4z], "-4": [neg(c4z)], "4/m": [c4z, inv], "422": [c4z, c2x], "4mm": [c4z, mx], "-42m": [neg(c4z), c2x], "4/mmm": [c4z, c2x, inv],
            "3": [c3h], "-3": [c3h, inv], "32": [c3h, c2a], "3m": [c3h, ma], "-3m": [c3h, c2a, inv],
            "6": [c6h], "-6": [neg(c6h)], "6/m": [c6h, inv], "622": [c6h, c2a], "6mm": [c6h, ma], "-6m2": [neg(c6h), ma], "6/mmm": [c6h, c2a, inv],
            "23": [c2z, c2x, c3d], "m-3": [c2z, c2x, c3d, inv], "432": [c4z, c3d], "-43m": [neg(c4z), c3d], "m-3m": [c4z, c3d, inv]}
    out = []
    for name in PG_NAMES:
        g = close_group(gens[name])
        hist = [0] * NCLASS
        for M in g:
            c = rot_class(M)
            assert c >= 0, (name, M)
            hist[c] += 1
        out.append((name, len(g), tuple(hist)))
    return out


def point_group(hist):
    hist = tuple(int(v) for v in hist)
    for i, (_, _, h) in enumerate(derive_point_groups()):
        if h == hist:
            return i + 1
    return 0


def crystal_system(pg):
    return 0 if pg < 1 else 1 if pg <= 2 else 2 if pg <= 5 else 3 if pg <= 8 else 4 if pg <= 15 else 5 if pg <= 20 else 6 if pg <= 27 else 7


# ---- mi_sym_find -------------------------------------------------------------------------------------------------------------------------------
def clear(x, bound, margin, what):
    if margin:
        assert abs(x - bound) > MARGIN, (what, x, bound)


def self_maps(L, inv, tol, cos_tol, margin=True):
    """(status, maps): the maps of the reduced cell onto itself, the matcher's enumeration with the absolute length rule."""
    ln, ct, maxlen = R.target(L)
    bound, pts = R.box_bounds(maxlen, inv, tol / min(ln))
    if pts < 0:
        return BOX_CAP, []
    cand = [[], [], []]
    for k0 in range(-bound[0], bound[0] + 1):
        for k1 in range(-bound[1], bound[1] + 1):
            for k2 in range(-bound[2], bound[2] + 1):
                v = [(float(k0) * L[c] + float(k1) * L[3 + c]) + float(k2) * L[6 + c] for c in range(3)]
                length = math.sqrt(R.dot3(v, v))
                for ax in range(3):
                    clear(abs(length - ln[ax]), tol, margin, "length")
                    if abs(length - ln[ax]) <= tol:
                        cand[ax].append(((k0, k1, k2), v, length))
    if any(len(c) > R.MAX_CAND for c in cand):
        return BOX_CAP, []
    maps = []
    for ki, vi, li in cand[0]:
        for kj, vj, lj in cand[1]:
            if not R.angle_ok(R.cos_of(vi, li, vj, lj), ct[2], cos_tol):
                continue
            for kk, vk, lk in cand[2]:
                if not R.angle_ok(R.cos_of(vi, li, vk, lk), ct[1], cos_tol) or not R.angle_ok(R.cos_of(vj, lj, vk, lk), ct[0], cos_tol):
                    continue
                M = list(ki) + list(kj) + list(kk)
                if R.idet3(M) in (1, -1):
                    maps.append(M)
    if not maps:
        return NO_LATTICE, []
    if len(maps) > R.MAX_MAPS:
        return MAP_CAP, []
    return OK, maps


def rigid_metric(L):
    return [R.dot3(L[3 * i:3 * i + 3], L[3 * j:3 * j + 3]) for i in range(3) for j in range(3)]


def nearest(G, f_atoms, images, T, want_u=True):
    """For translations T [J, 3]: (index [J, nb] of the nearest atom of f_atoms [na, 3] to each image images [nb, 3] + T[j] -- the first
    minimum in ascending order --, its squared distance clamped at 0, the displacement u [J, nb, 3]).  sm_pair_cost's operation order."""
    T = np.asarray(T, np.float64).reshape(-1, 3)
    d = (images[None, None, :, :] + T[:, None, None, :]) - f_atoms[None, :, None, :]   # [J, atom, image, 3]
    D = d - np.floor(d + 0.5)
    best = np.full(D.shape[:3], R.INF)
    u = D.copy() if want_u else None
    for kx in (-1, 0, 1):
        for ky in (-1, 0, 1):
            for kz in (-1, 0, 1):
                x, y, z = D[..., 0] + float(kx), D[..., 1] + float(ky), D[..., 2] + float(kz)
                q = R.quad(G, x, y, z)
                better = q < best
                best = np.where(better, q, best)
                if want_u:
                    u = np.where(better[..., None], np.stack([x, y, z], axis=-1), u)
    at = np.argmin(best, axis=1)                                                       # [J, image]: the first minimum
    d2 = np.take_along_axis(best, at[:, None, :], axis=1)[:, 0, :]
    uu = np.take_along_axis(u, at[:, None, :, None], axis=1)[:, 0, :, :] if want_u else None
    return at, np.where(d2 > 0.0, d2, 0.0), uu


def failed(status):
    return {"info": [0] * (NINFO - 1) + [status], "rot_hist": [0] * NCLASS, "rot": [], "trans": [], "dev": [], "ptrans": []}


def find_one(P, b, tol, cos_tol, margin=True):
    """The outputs of mi_sym_find for crystal b of the prepared set P (tests/sm_ref64.prepare) as a dict: info [8], rot_hist [10] and the
    written rows of rot, trans, dev (at most MAX_OPS) and ptrans."""
    pinfo = P["info"][b]
    if pinfo[3] != R.PREP_OK:
        return failed(NOT_PREPARED)
    tol = float(tol)
    if not (tol >= 0.0 and tol <= 1.0):
        return failed(BAD_TOL)
    n, nspec, rarest = int(pinfo[0]), int(pinfo[1]), int(pinfo[2])
    L, inv = [float(x) for x in P["lat"][b]], [float(x) for x in P["inv"][b]]
    st, maps = self_maps(L, inv, tol, cos_tol, margin)
    if st != OK:
        return failed(st)
    n0 = int(P["offsets"][b])
    f = np.array(P["frac"][n0:n0 + n], np.float64)
    so = [int(v) for v in P["spec_off"][b]]
    r0, ntrans = so[rarest], so[rarest + 1] - so[rarest]
    G = rigid_metric(L)
    out = {"rot": [], "trans": [], "dev": [], "ptrans": []}
    n_ops = n_trans = pg_order = status = 0
    hist = [0] * NCLASS
    for M in maps:
        fp = R.map_frac(f, R.map_inverse(M))
        T = np.array([[float(f[r0 + j, c]) - float(fp[r0, c]) for c in range(3)] for j in range(ntrans)])
        tgt, dist, u = np.zeros((ntrans, n), np.int64), np.zeros((ntrans, n)), np.zeros((ntrans, n, 3))
        for s in range(nspec):
            b0, b1 = so[s], so[s + 1]
            at, d2, uu = nearest(G, f[b0:b1], fp[b0:b1], T, want_u=M == IDENT)
            tgt[:, b0:b1], dist[:, b0:b1] = b0 + at, np.sqrt(d2)
            if M == IDENT:
                u[:, b0:b1] = uu
        first = True
        for j in range(ntrans):
            if margin:
                assert (np.abs(dist[j] - tol) > MARGIN).all(), ("distance", b, M, j)
            within = bool((dist[j] <= tol).all())
            bij = len(set(int(v) for v in tgt[j])) == n
            if within and not bij:
                status |= AMBIGUOUS
            if not (within and bij):
                continue
            if first:
                first = False
                pg_order += 1
                c = rot_class(M)
                if c < 0:
                    status |= NOT_A_GROUP
                else:
                    hist[c] += 1
            if n_ops < MAX_OPS:
                out["rot"].append(list(M))
                out["trans"].append([R.wrap01(float(T[j, c])) for c in range(3)])
                out["dev"].append(float(dist[j].max()))
            n_ops += 1
            if M == IDENT:
                s0 = s1 = s2 = 0.0
                for a in range(n):
                    s0, s1, s2 = s0 + float(u[j, a, 0]), s1 + float(u[j, a, 1]), s2 + float(u[j, a, 2])
                mean = [s0 / float(n), s1 / float(n), s2 / float(n)]
                out["ptrans"].append([R.wrap01(float(T[j, c]) - mean[c]) for c in range(3)])
                n_trans += 1
    if n_ops > MAX_OPS:
        status |= OPS_CAP
    if n_ops != pg_order * n_trans:
        status |= NOT_A_GROUP
    pg = point_group(hist)
    if pg == 0:
        status |= NOT_A_GROUP
    out["info"] = [n_ops, n_trans, len(maps), pg_order, pg, crystal_system(pg), 1 if hist[4] > 0 else 0, status]
    out["rot_hist"] = hist
    return out


def empty_find(B, value=0):
    return {"info": np.full((B, NINFO), value, np.int32), "rot_hist": np.full((B, NCLASS), value, np.int32), "rot": np.full((B, MAX_OPS, 9), value, np.int32),
            "trans": np.full((B, MAX_OPS, 3), float(value)), "dev": np.full((B, MAX_OPS), float(value)), "ptrans": np.full((B, MAX_TRANS, 3), float(value))}


def find(P, tol, cos_tol, fill=0, margin=True):
    """mi_sym_find over a prepared set: the arrays of mi_sym_out; rows the kernel does not write keep `fill`."""
    B = len(P["info"])
    out = empty_find(B, fill)
    for b in range(B):
        r = find_one(P, b, tol[b], cos_tol, margin)
        out["info"][b], out["rot_hist"][b] = r["info"], r["rot_hist"]
        for k in ("rot", "trans", "dev", "ptrans"):
            if len(r[k]):
                out[k][b, :len(r[k])] = r[k]
    return out


def tolerances(offsets, lat, symprec):
    """symprec / (V_b / n_b)^(1/3) per crystal, V_b in float64 from the float32 cell: the host's conversion (matinvent_amd/symmetry.py)."""
    lat = np.asarray(lat, np.float32).reshape(-1, 9).astype(np.float64)
    out = np.ones(len(lat))
    for b in range(len(lat)):
        n, v = int(offsets[b + 1]) - int(offsets[b]), abs(R.det3([float(x) for x in lat[b]]))
        if n >= 1 and math.isfinite(v) and v > 0.0:
            out[b] = float(symprec) / (v / n) ** (1.0 / 3.0)
    return out


# ---- mi_sym_primitive --------------------------------------------------------------------------------------------------------------------------
def centre(x):
    return x - math.floor(x + 0.5)


def prim_cand(ptrans, ntr, e):
    return [centre(float(ptrans[e][c])) for c in range(3)] if e < ntr else [1.0 if e - ntr == c else 0.0 for c in range(3)]


def primitive(P, types, frac, lat, S, fill=0, margin=True):
    """mi_sym_primitive: dict of prim_offsets [B + 1], prim_count, prim_status [B], prim_det [B], types [N], frac [N, 3] float32, lat [B, 9]
    float32.  S: the arrays of find()."""
    types, frac = np.asarray(types, np.int32), np.asarray(frac, np.float32).reshape(-1, 3)
    lat = np.asarray(lat, np.float32).reshape(-1, 9)
    B, N = len(lat), len(types)
    out = {"types": np.full(N, fill, np.int32), "frac": np.full((N, 3), fill, np.float32), "lat": lat.copy(), "prim_count": np.zeros(B, np.int32),
           "prim_status": np.zeros(B, np.int32), "prim_det": np.ones(B)}
    kept_rows = []
    for b in range(B):
        n0, n1 = int(P["offsets"][b]), int(P["offsets"][b + 1])
        st, ntr = int(S["info"][b][7]), int(S["info"][b][1])
        if not (0 <= n0 <= n1 <= N):
            kept_rows.append((np.zeros(0, np.int32), np.zeros((0, 3), np.float32)))
            out["prim_status"][b] = st
            continue
        n = n1 - n0
        same = (types[n0:n1].copy(), frac[n0:n1].copy())
        if (st & ~OPS_CAP) != OK or ntr <= 1 or ntr > MAX_TRANS or n > R.MAX_ATOMS:
            kept_rows.append(same)
            out["prim_count"][b], out["prim_status"][b] = n, st
            continue
        pt = S["ptrans"][b]
        m, found = ntr + 3, None
        for i, j, k in itertools.combinations(range(m), 3):
            Pm = prim_cand(pt, ntr, i) + prim_cand(pt, ntr, j) + prim_cand(pt, ntr, k)
            x = abs(abs(R.det3(Pm)) * float(ntr) - 1.0)
            clear(x, 0.1, margin, "determinant")
            if x < 0.1:
                found = Pm
                break
        if found is None:
            kept_rows.append(same)
            out["prim_count"][b], out["prim_status"][b] = n, st | PRIM_FAIL
            continue
        det = R.det3(found)
        Pinv = R.inv3(found, det)
        f = np.array(P["frac"][n0:n1], np.float64)
        so = [int(v) for v in P["spec_off"][b]]
        G = rigid_metric([float(x) for x in P["lat"][b]])
        keep = np.ones(n, bool)
        for s in range(int(P["info"][b][1])):
            b0, b1 = so[s], so[s + 1]
            at, _, _ = nearest(G, f[b0:b1], f[b0:b1], np.array(pt[1:ntr]), want_u=False)
            keep[b0:b1] = ((b0 + at) > np.arange(b0, b1)[None, :]).all(axis=0)
        if int(keep.sum()) * ntr != n:
            kept_rows.append(same)
            out["prim_count"][b], out["prim_status"][b] = n, st | PRIM_FAIL
            continue
        perm = np.asarray(P["perm"][n0:n1])
        src = np.zeros(n, np.int64)
        src[perm] = np.arange(n)
        zs, fs = [], []
        for c in range(n):   # the caller's order
            a = int(src[c])
            if keep[a]:
                row = []
                for col in range(3):
                    w = np.float32(R.wrap01((float(f[a, 0]) * Pinv[col] + float(f[a, 1]) * Pinv[3 + col]) + float(f[a, 2]) * Pinv[6 + col]))
                    row.append(np.float32(0.0) if w >= np.float32(1.0) else w)
                zs.append(types[n0 + c]), fs.append(row)
        ok, T, Lr = R.reduce_cell([float(v) for v in lat[b]])
        assert ok
        out["lat"][b] = [np.float32((found[3 * i] * Lr[c] + found[3 * i + 1] * Lr[3 + c]) + found[3 * i + 2] * Lr[6 + c]) for i in range(3) for c in range(3)]
        kept_rows.append((np.asarray(zs, np.int32), np.asarray(fs, np.float32).reshape(-1, 3)))
        out["prim_count"][b], out["prim_status"][b], out["prim_det"][b] = len(zs), st, abs(det)
    off = np.concatenate([[0], np.cumsum(out["prim_count"])]).astype(np.int32)
    out["prim_offsets"] = off
    for b, (z, fr) in enumerate(kept_rows):
        lo, hi = int(off[b]), min(int(off[b]) + len(z), N)
        if hi > lo:
            out["types"][lo:hi], out["frac"][lo:hi] = z[:hi - lo], fr[:hi - lo]
    return out


# ---- the certificate: from the input alone -----------------------------------------------------------------------------------------------------
def certificate(crystal, symprec, ops, complete):
    """ops: [(W [9], t [3])] for `crystal` = (lattice, types, frac), in the basis of the PREPARED set, so the caller hands the prepared
    cell and coordinates in as the crystal.  Checks, in float64 with numpy's own operations (not the restatement's): every (W, t) maps
    every atom onto an atom of its species within symprec; W L is an isometric image of L within the tolerance; with `complete`, the set is
    closed under composition modulo lattice translations."""
    L, z, f = np.asarray(crystal[0], np.float64).reshape(3, 3), np.asarray(crystal[1]), np.asarray(crystal[2], np.float64).reshape(-1, 3)
    G = L @ L.T
    shifts = np.array(list(itertools.product((-1, 0, 1), repeat=3)), np.float64)
    lens = np.sqrt(np.diag(G))

    def dist(d):
        d = d - np.round(d)
        v = (d[None, :] + shifts) @ L
        return np.sqrt((v * v).sum(1).min())

    for W, t in ops:
        Wm = np.asarray(W, np.float64).reshape(3, 3)
        assert round(abs(np.linalg.det(Wm))) == 1
        WL = Wm @ L
        assert np.abs(np.sqrt(np.diag(WL @ WL.T)) - lens).max() <= symprec * (1 + 1e-9)
        img = f @ np.linalg.inv(Wm) + np.asarray(t)[None, :]
        for a in range(len(z)):
            assert min(dist(img[a] - f[b]) for b in range(len(z)) if z[b] == z[a]) <= symprec * (1 + 1e-9), (W, t, a)
    if complete:
        def key(W, t):
            return tuple(int(v) for v in W)

        by_rot = {}
        for W, t in ops:
            by_rot.setdefault(key(W, t), []).append(np.asarray(t, np.float64))
        for W1, t1 in ops:
            for W2, t2 in ops:
                # f -> (f W1^-1 + t1) W2^-1 + t2 = f (W2 W1)^-1 + (t1 W2^-1 + t2)
                W = (np.asarray(W2).reshape(3, 3) @ np.asarray(W1).reshape(3, 3)).reshape(9)
                t = np.asarray(t1) @ np.linalg.inv(np.asarray(W2, np.float64).reshape(3, 3)) + np.asarray(t2)
                cands = by_rot.get(tuple(int(v) for v in W))
                assert cands is not None, (W1, W2)
                assert min(dist(t - c) for c in cands) <= 2 * symprec, (W1, t1, W2, t2)
    return True
