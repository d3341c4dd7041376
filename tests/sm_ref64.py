"""The structure matcher of DESIGN 49 restated in numpy / plain Python float64, operation for operation: the executable form of the
definition, and the reference every output of mi_sm_prepare and mi_sm_match is held to bit for bit.  Scalars are Python floats (IEEE
double, one rounding per operation), vectors are numpy float64 with the same operation order per element; sqrt and floor are exact in
both.  Nothing here is fast: the tests keep their shapes small."""
import math

import numpy as np

MAX_ATOMS, MAX_SPECIES, MAX_Z, MAX_MAPS, MAX_CAND, BOX_CAP = 64, 16, 118, 256, 128, 32768
REDUCE_SWEEPS, T_MAX, ROOT_ITERS, MIN_VOLUME = 64, 1 << 20, 200, 0.1
PREP_OK, PREP_BAD_INPUT, PREP_TOO_MANY_ATOMS, PREP_TOO_MANY_SPECIES, PREP_DEGENERATE_CELL, PREP_REDUCE_CAP = range(6)
OK, NO_LATTICE, BOX_CAP_HIT, MAP_CAP_HIT, SPECIES_MISMATCH, BAD_PAIR, NOT_PREPARED = range(7)
INF = float("inf")


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def det3(L):
    return (L[0] * (L[4] * L[8] - L[5] * L[7]) - L[1] * (L[3] * L[8] - L[5] * L[6])) + L[2] * (L[3] * L[7] - L[4] * L[6])


def inv3(L, det):
    return [(L[4] * L[8] - L[5] * L[7]) / det, (L[2] * L[7] - L[1] * L[8]) / det, (L[1] * L[5] - L[2] * L[4]) / det,
            (L[5] * L[6] - L[3] * L[8]) / det, (L[0] * L[8] - L[2] * L[6]) / det, (L[2] * L[3] - L[0] * L[5]) / det,
            (L[3] * L[7] - L[4] * L[6]) / det, (L[1] * L[6] - L[0] * L[7]) / det, (L[0] * L[4] - L[1] * L[3]) / det]


def idet3(M):
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6])


def iadj3(M):
    return [M[4] * M[8] - M[5] * M[7], M[2] * M[7] - M[1] * M[8], M[1] * M[5] - M[2] * M[4],
            M[5] * M[6] - M[3] * M[8], M[0] * M[8] - M[2] * M[6], M[2] * M[3] - M[0] * M[5],
            M[3] * M[7] - M[4] * M[6], M[1] * M[6] - M[0] * M[7], M[0] * M[4] - M[1] * M[3]]


def cuberoot(r):
    x = r if r > 1.0 else 1.0
    for _ in range(ROOT_ITERS):
        nx = ((x + x) + r / (x * x)) / 3.0
        if not nx < x:
            break
        x = nx
    return x


def trow(T, L0, i):
    return [(float(T[3 * i]) * L0[c] + float(T[3 * i + 1]) * L0[3 + c]) + float(T[3 * i + 2]) * L0[6 + c] for c in range(3)]


def reduce_cell(L0):
    """(ok, T, L): the greedy Minkowski pair reduction of csrc/sm_lattice.h."""
    T = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    L = list(L0)
    for _ in range(REDUCE_SWEEPS):
        changed = False
        for i in range(3):
            for j in ((1, 2), (0, 2), (0, 1))[i]:
                q = dot3(L[3 * i:3 * i + 3], L[3 * j:3 * j + 3]) / dot3(L[3 * j:3 * j + 3], L[3 * j:3 * j + 3])
                m = math.floor(q + 0.5) if math.isfinite(q) else q
                if m != 0.0 and abs(m) <= T_MAX:
                    Tn = list(T)
                    for c in range(3):
                        t = float(T[3 * i + c]) - m * float(T[3 * j + c])
                        if abs(t) > T_MAX:
                            return False, T, L
                        Tn[3 * i + c] = int(t)
                    row = trow(Tn, L0, i)
                    if dot3(row, row) < dot3(L[3 * i:3 * i + 3], L[3 * i:3 * i + 3]):
                        T[3 * i:3 * i + 3] = Tn[3 * i:3 * i + 3]
                        L[3 * i:3 * i + 3] = row
                        changed = True
            j, k = ((1, 2), (0, 2), (0, 1))[i]
            best, bs, bt = dot3(L[3 * i:3 * i + 3], L[3 * i:3 * i + 3]), 0, 0
            for s in (-1, 0, 1):
                for t in (-1, 0, 1):
                    if s == 0 and t == 0:
                        continue
                    Tn = list(T)
                    for c in range(3):
                        Tn[3 * i + c] = T[3 * i + c] + s * T[3 * j + c] + t * T[3 * k + c]
                    row = trow(Tn, L0, i)
                    l2 = dot3(row, row)
                    if l2 < best:
                        best, bs, bt = l2, s, t
            if bs != 0 or bt != 0:
                for c in range(3):
                    T[3 * i + c] = T[3 * i + c] + bs * T[3 * j + c] + bt * T[3 * k + c]
                if any(abs(T[3 * i + c]) > T_MAX for c in range(3)):
                    return False, T, L
                L[3 * i:3 * i + 3] = trow(T, L0, i)
                changed = True
        if not changed:
            return True, T, L
    return False, T, L


def wrap01(x):
    w = x - math.floor(x)
    return 0.0 if w >= 1.0 else w


def prepare_cell(lat32, n):
    """(status, T, Ls, inv) from the float32 cell [9]."""
    L0 = [float(v) for v in lat32]
    if not abs(det3(L0)) >= MIN_VOLUME:
        return PREP_DEGENERATE_CELL, None, None, None
    ok, T, L = reduce_cell(L0)
    if not ok:
        return PREP_REDUCE_CAP, None, None, None
    s = cuberoot(float(n) / abs(det3(L)))
    Ls = [v * s for v in L]
    return PREP_OK, T, Ls, inv3(Ls, det3(Ls))


def prepare(offsets, types, frac, lat, fill=None):
    """The arrays of mi_sm_prepare for a batch: dict of lat [B, 9], inv [B, 9], frac [N, 3], types [N], perm [N], spec_Z [B, 16],
    spec_off [B, 17], info [B, 4].  Rows the kernel does not write keep `fill` (a dict of the same arrays) or zeros."""
    offsets, types = np.asarray(offsets, np.int64), np.asarray(types, np.int64)
    frac, lat = np.asarray(frac, np.float32).reshape(-1, 3), np.asarray(lat, np.float32).reshape(-1, 9)
    B, N = len(offsets) - 1, len(types)
    out = {"lat": np.zeros((B, 9)), "inv": np.zeros((B, 9)), "frac": np.zeros((N, 3)), "types": np.zeros(N, np.int32), "perm": np.zeros(N, np.int32),
           "spec_Z": np.zeros((B, MAX_SPECIES), np.int32), "spec_off": np.zeros((B, MAX_SPECIES + 1), np.int32), "info": np.zeros((B, 4), np.int32)}
    if fill is not None:
        out = {k: np.array(fill[k], copy=True) for k in out}
    out["offsets"] = offsets.astype(np.int32)
    for b in range(B):
        n0, n1 = int(offsets[b]), int(offsets[b + 1])
        if not (0 <= n0 <= n1 <= N):
            out["info"][b] = (0, 0, 0, PREP_BAD_INPUT)
            continue
        n = n1 - n0
        if n < 1 or n > MAX_ATOMS:
            out["info"][b] = (n, 0, 0, PREP_BAD_INPUT if n < 1 else PREP_TOO_MANY_ATOMS)
            continue
        z, f = types[n0:n1], frac[n0:n1]
        if not (np.isfinite(lat[b]).all() and np.isfinite(f).all() and ((z >= 1) & (z <= MAX_Z)).all()):
            out["info"][b] = (n, 0, 0, PREP_BAD_INPUT)
            continue
        species = sorted(set(int(v) for v in z))
        if len(species) > MAX_SPECIES:
            out["info"][b] = (n, 0, 0, PREP_TOO_MANY_SPECIES)
            continue
        st, T, Ls, inv = prepare_cell(lat[b], n)
        if st != PREP_OK:
            out["info"][b] = (n, 0, 0, st)
            continue
        out["lat"][b], out["inv"][b] = Ls, inv
        order = np.argsort(z, kind="stable")
        A = iadj3(T)
        for pos, a in enumerate(order):
            f0, f1, f2 = float(f[a, 0]), float(f[a, 1]), float(f[a, 2])
            out["frac"][n0 + pos] = [wrap01((f0 * float(A[c]) + f1 * float(A[3 + c])) + f2 * float(A[6 + c])) for c in range(3)]
            out["types"][n0 + pos], out["perm"][n0 + pos] = z[a], a
        zs = z[order]
        offs = [int(np.searchsorted(zs, s, "left")) for s in species]
        out["spec_Z"][b] = species + [0] * (MAX_SPECIES - len(species))
        out["spec_off"][b] = offs + [n] * (MAX_SPECIES + 1 - len(species))
        so = out["spec_off"][b]
        rarest = 0
        for s in range(1, len(species)):
            if so[s + 1] - so[s] < so[rarest + 1] - so[rarest]:
                rarest = s
        out["info"][b] = (n, len(species), rarest, PREP_OK)
    return out


# ---- the lattice maps ---------------------------------------------------------------------------------------------------------------------------
def clamp1(c):
    return 1.0 if c > 1.0 else (-1.0 if c < -1.0 else c)


def cos_of(u, lu, v, lv):
    return clamp1(dot3(u, v) / (lu * lv))


def target(L1):
    ln = [math.sqrt(dot3(L1[3 * i:3 * i + 3], L1[3 * i:3 * i + 3])) for i in range(3)]
    a, b, c = L1[0:3], L1[3:6], L1[6:9]
    return ln, [cos_of(b, ln[1], c, ln[2]), cos_of(a, ln[0], c, ln[2]), cos_of(a, ln[0], b, ln[1])], max(ln)


def box_bounds(maxlen, inv2, ltol):
    """(bound [3], points) or (bound, -1) over the cap."""
    bound, pts, over = [0, 0, 0], 1, False
    for i in range(3):
        bl = math.sqrt((inv2[i] * inv2[i] + inv2[3 + i] * inv2[3 + i]) + inv2[6 + i] * inv2[6 + i])
        b = math.floor(((1.0 + ltol) * maxlen) * bl) if math.isfinite(bl) else INF
        over = over or not b <= BOX_CAP
        bound[i] = 0 if over else int(b)
        pts *= 2 * bound[i] + 1
        over = over or pts > BOX_CAP
    return bound, (-1 if over else pts)


def angle_ok(c, ct, cos_tol):
    return c * ct + math.sqrt(1.0 - c * c) * math.sqrt(1.0 - ct * ct) >= cos_tol


def candidates(L1, L2, inv2, ltol, bound_scale=1):
    """(status, [three lists of (k, v, len)]): the candidate vectors per axis in lexicographic order of k.  bound_scale widens the box
    (the enumeration-bound test)."""
    ln, _, maxlen = target(L1)
    bound, pts = box_bounds(maxlen, inv2, ltol)
    if pts < 0:
        return BOX_CAP_HIT, None
    bound = [b * bound_scale for b in bound]
    cand = [[], [], []]
    for k0 in range(-bound[0], bound[0] + 1):
        for k1 in range(-bound[1], bound[1] + 1):
            for k2 in range(-bound[2], bound[2] + 1):
                v = [(float(k0) * L2[c] + float(k1) * L2[3 + c]) + float(k2) * L2[6 + c] for c in range(3)]
                length = math.sqrt(dot3(v, v))
                for ax in range(3):
                    if abs(length / ln[ax] - 1.0) <= ltol:
                        cand[ax].append(((k0, k1, k2), v, length))
    return OK, cand


def lattice_maps(L1, L2, inv2, ltol, cos_tol):
    """(status, maps): maps a list of 9-int lists, in order."""
    st, cand = candidates(L1, L2, inv2, ltol)
    if st != OK:
        return st, []
    if any(len(c) > MAX_CAND for c in cand):
        return BOX_CAP_HIT, []
    _, ct, _ = target(L1)
    maps = []
    for ki, vi, li in cand[0]:
        for kj, vj, lj in cand[1]:
            if not angle_ok(cos_of(vi, li, vj, lj), ct[2], cos_tol):
                continue
            for kk, vk, lk in cand[2]:
                if not angle_ok(cos_of(vi, li, vk, lk), ct[1], cos_tol) or not angle_ok(cos_of(vj, lj, vk, lk), ct[0], cos_tol):
                    continue
                M = list(ki) + list(kj) + list(kk)
                if idet3(M) in (1, -1):
                    maps.append(M)
    if not maps:
        return NO_LATTICE, []
    if len(maps) > MAX_MAPS:
        return MAP_CAP_HIT, maps[:MAX_MAPS]
    return OK, maps


# ---- one item --------------------------------------------------------------------------------------------------------------------------------
def metric(L1, L2, M):
    ML = [(float(M[3 * i]) * L2[c] + float(M[3 * i + 1]) * L2[3 + c]) + float(M[3 * i + 2]) * L2[6 + c] for i in range(3) for c in range(3)]
    return [(dot3(L1[3 * i:3 * i + 3], L1[3 * j:3 * j + 3]) + dot3(ML[3 * i:3 * i + 3], ML[3 * j:3 * j + 3])) * 0.5 for i in range(3) for j in range(3)]


def map_inverse(M):
    d = idet3(M)
    return [a * d for a in iadj3(M)]


def vwrap01(x):
    w = x - np.floor(x)
    return np.where(w >= 1.0, 0.0, w)


def map_frac(f2, Mi):
    """wrap(f2 M^-1) for rows f2 [n, 3]."""
    return np.stack([vwrap01((f2[:, 0] * float(Mi[c]) + f2[:, 1] * float(Mi[3 + c])) + f2[:, 2] * float(Mi[6 + c])) for c in range(3)], axis=1)


def quad(G, x, y, z):
    g0 = (G[0] * x + G[1] * y) + G[2] * z
    g1 = (G[3] * x + G[4] * y) + G[5] * z
    g2 = (G[6] * x + G[7] * y) + G[8] * z
    return (x * g0 + y * g1) + z * g2


def pair_costs(G, f1, f2p, t, images=1):
    """(cost [na, nb], u [na, nb, 3]): rows the query's atoms f1 [na, 3], columns the candidate's f2p [nb, 3]; the first minimum over the
    (2 images + 1)^3 neighbouring images in lexicographic order."""
    d = (f2p[None, :, :] + np.asarray(t)[None, None, :]) - f1[:, None, :]
    D = d - np.floor(d + 0.5)
    best = np.full(D.shape[:2], INF)
    u = D.copy()
    r = range(-images, images + 1)
    for kx in r:
        for ky in r:
            for kz in r:
                x, y, z = D[..., 0] + float(kx), D[..., 1] + float(ky), D[..., 2] + float(kz)
                q = quad(G, x, y, z)
                better = q < best
                best = np.where(better, q, best)
                u = np.where(better[..., None], np.stack([x, y, z], axis=-1), u)
    return best, u


def assign(cost):
    """col4row of the square cost matrix by shortest augmenting paths, rows ascending, every argmin to the lowest column; None when a cost is
    not a number.  The steps and the operation order of csrc/sm_assign.h sm_assign_serial."""
    cost = np.asarray(cost, np.float64)
    nb = len(cost)
    u, v = np.zeros(nb), np.zeros(nb)
    row4col, col4row, path = -np.ones(nb, np.int64), -np.ones(nb, np.int64), -np.ones(nb, np.int64)
    for cur in range(nb):
        shortest = np.full(nb, INF)
        SR, SC = np.zeros(nb, bool), np.zeros(nb, bool)
        min_val, i, sink = 0.0, cur, -1
        while sink < 0:
            SR[i] = True
            r = ((min_val + cost[i]) - u[i]) - v
            upd = ~SC & (r < shortest)
            shortest = np.where(upd, r, shortest)
            path = np.where(upd, i, path)
            masked = np.where(SC, np.nan, shortest)
            if np.isnan(masked).all():
                return None
            bv = np.nanmin(masked)
            hits = np.nonzero(~SC & (shortest == bv))[0]
            if len(hits) == 0:
                return None
            bj = int(hits[0])
            if not bv < INF:
                return None
            min_val = float(bv)
            SC[bj] = True
            if row4col[bj] < 0:
                sink = bj
            else:
                i = int(row4col[bj])
        rows = SR.copy()
        rows[cur] = False
        u[cur] = u[cur] + min_val
        u[rows] = u[rows] + (min_val - shortest[col4row[rows]])
        v[SC] = v[SC] - (min_val - shortest[SC])
        j = sink
        while True:
            r_ = int(path[j])
            row4col[j] = r_
            col4row[r_], j = j, int(col4row[r_])
            if r_ == cur:
                break
    return col4row


def eval_item(L1, L2, f1, f2, spec_off, nspec, r0, M, j, images=1):
    """(rms, max_dist, col [n] sorted candidate index per sorted query atom, u [n, 3]) of one (map, translation) item; rms = inf when an
    assignment failed."""
    n = len(f1)
    G = metric(L1, L2, M)
    f2p = map_frac(f2, map_inverse(M))
    t = [float(f1[r0 + j, c]) - float(f2p[r0, c]) for c in range(3)]
    col, uvec = np.zeros(n, np.int64), np.zeros((n, 3))
    for s in range(nspec):
        b0, b1 = int(spec_off[s]), int(spec_off[s + 1])
        cost, u = pair_costs(G, f1[b0:b1], f2p[b0:b1], t, images)
        c4r = assign(cost)
        if c4r is None:
            return INF, INF, None, None
        col[b0:b1] = b0 + c4r
        uvec[b0:b1] = u[np.arange(b1 - b0), c4r]
    s0 = s1 = s2 = 0.0
    for a in range(n):
        s0, s1, s2 = s0 + float(uvec[a, 0]), s1 + float(uvec[a, 1]), s2 + float(uvec[a, 2])
    mean = [s0 / float(n), s1 / float(n), s2 / float(n)]
    d2 = quad(G, uvec[:, 0] - mean[0], uvec[:, 1] - mean[1], uvec[:, 2] - mean[2])
    ssum, m = 0.0, 0.0
    for a in range(n):
        ssum = ssum + float(d2[a])
        m = float(d2[a]) if d2[a] > m else m
    ms = ssum / float(n)
    return math.sqrt(ms if ms > 0.0 else 0.0), math.sqrt(m), col, uvec


def failed(status, n_maps=0):
    return {"rms": INF, "max_dist": INF, "best_map": [0] * 9, "best_trans": -1, "n_maps": n_maps, "n_items": 0, "status": status,
            "perm": [-1] * MAX_ATOMS, "maps": []}


def match_pair(A, q, Bset, c, ltol=0.2, cos_tol=math.cos(math.radians(5.0))):
    """The outputs of mi_sm_match for one pair (query q of prepared set A, candidate c of prepared set Bset) as a dict."""
    if not (0 <= q < len(A["info"]) and 0 <= c < len(Bset["info"])):
        return failed(BAD_PAIR)
    ia, ib = A["info"][q], Bset["info"][c]
    if ia[3] != PREP_OK or ib[3] != PREP_OK:
        return failed(NOT_PREPARED)
    if not (ia[0] == ib[0] and ia[1] == ib[1] and (A["spec_Z"][q] == Bset["spec_Z"][c]).all() and (A["spec_off"][q][:MAX_SPECIES] == Bset["spec_off"][c][:MAX_SPECIES]).all()):
        return failed(SPECIES_MISMATCH)
    n, nspec = int(ia[0]), int(ia[1])
    L1, L2, inv2 = [float(x) for x in A["lat"][q]], [float(x) for x in Bset["lat"][c]], [float(x) for x in Bset["inv"][c]]
    st, maps = lattice_maps(L1, L2, inv2, ltol, cos_tol)
    if st != OK:
        return failed(st, MAX_MAPS if st == MAP_CAP_HIT else 0)
    n0a, n0b = int(A["offsets"][q]), int(Bset["offsets"][c])
    f1, f2 = A["frac"][n0a:n0a + n], Bset["frac"][n0b:n0b + n]
    spec_off = A["spec_off"][q]
    rarest = int(ib[2])
    r0, ntrans = int(spec_off[rarest]), int(spec_off[rarest + 1] - spec_off[rarest])
    NO_ITEM = 0x7fffffff
    best, best_m, best_i, best_col = INF, INF, NO_ITEM, None
    for m, M in enumerate(maps):
        for j in range(ntrans):
            rms, md, col, _ = eval_item(L1, L2, f1, f2, spec_off, nspec, r0, M, j)
            item = m * ntrans + j
            if rms < best or (rms == best and item < best_i):   # (value, item) ascending: the first minimum
                best, best_m, best_i, best_col = rms, md, item, col
    out = {"rms": best, "max_dist": best_m, "n_maps": len(maps), "n_items": len(maps) * ntrans, "status": OK, "maps": maps}
    if best_i == NO_ITEM:
        out.update(best_map=[0] * 9, best_trans=-1, perm=[-1] * MAX_ATOMS, rms=INF, max_dist=INF)
        return out
    out["best_map"], out["best_trans"] = maps[best_i // ntrans], best_i % ntrans
    perm = [-1] * MAX_ATOMS
    if best_col is not None:
        for a in range(n):
            perm[int(A["perm"][n0a + a])] = int(Bset["perm"][n0b + int(best_col[a])])
    out["perm"] = perm
    return out
