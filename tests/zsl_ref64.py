"""The substrate matcher restated in numpy float64 (include/matinvent_hip_zsl.h, matinvent_amd/csrc/zsl_match.h), written from the
definition and operation for operation: every sum and product in the header's order, no fused multiply-add.  `analyze` is what the device
computes (planes, tables, search, reduce) and records the smallest |quantity - tolerance| over every decision it takes (`margin`);
`brute` is a second, independent routine: plain loops over all planes and all Hermite normal forms, a recursive reduction, no early exit,
every match kept in one list.  `write_case` / `read_out` are the files of scripts/zsl_host_check.cpp."""
import math
import struct

import numpy as np

MAX_MULT, MAX_MILLER, REDUCE_ITERS, TABLE, ROW_D, ROW_I = 63, 8, 64, 3276, 10, 20
OK, NO_MATCH, MULT_CAP, REDUCE_CAP, BAD_CELL = 0, 1, 2, 3, 4
SIGMA = [0] + [sum(n // d for d in range(1, n + 1) if n % d == 0) for n in range(1, MAX_MULT + 2)]
OFFSET = [0] + [sum(SIGMA[1:n]) for n in range(1, MAX_MULT + 2)]
assert OFFSET[MAX_MULT + 1] == TABLE and max(SIGMA[:MAX_MULT + 1]) == 168
DEFAULTS = dict(max_area=400.0, max_area_ratio_tol=0.09, max_length_tol=0.03, max_angle_tol=0.01)


def planes(m=1):
    """(h, k, l) in [-m, m]^3, not all zero, coprime, the first non-zero entry positive; ascending lexicographic order."""
    out = []
    for h in range(-m, m + 1):
        for k in range(-m, m + 1):
            for l in range(-m, m + 1):
                if (h, k, l) == (0, 0, 0) or math.gcd(math.gcd(abs(h), abs(k)), abs(l)) != 1:
                    continue
                if next(v for v in (h, k, l) if v != 0) > 0:
                    out.append((h, k, l))
    return out


def _tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def egcd(h, k):
    """(g, p, q): g = gcd(h, k) > 0 and p h + q k = g; the quotients truncate toward zero."""
    r0, r1, s0, s1, t0, t1 = h, k, 1, 0, 0, 1
    while r1 != 0:
        qu = _tdiv(r0, r1)
        r0, r1, s0, s1, t0, t1 = r1, r0 - qu * r1, s1, s0 - qu * s1, t1, t0 - qu * t1
    if r0 < 0:
        r0, s0, t0 = -r0, -s0, -t0
    return r0, s0, t0


def basis(hkl):
    h, k, l = hkl
    if h == 0 and k == 0:
        return (1, 0, 0), (0, 1, 0)
    g, p, q = egcd(h, k)
    return (_tdiv(-k, g), _tdiv(h, g), 0), (-p * l, -q * l, g)


def hnfs(n):
    return [(i, j, n // i) for i in range(1, n + 1) if n % i == 0 for j in range(n // i)]


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def reduce_pairs(a, b):
    """The pair reduction on arrays [K, 3]: per pair the first rule that applies, at most 64 applications; (a, b, ended [K])."""
    a, b = np.array(a, np.float64).reshape(-1, 3), np.array(b, np.float64).reshape(-1, 3)
    live = np.ones(len(a), bool)
    for _ in range(REDUCE_ITERS):
        if not live.any():
            break
        na, nb = _dot(a, a), _dot(b, b)
        p, m = b + a, b - a
        r1 = live & (_dot(a, b) < 0.0)
        r2 = live & ~r1 & (na > nb)
        r3 = live & ~r1 & ~r2 & (nb > _dot(p, p))
        r4 = live & ~r1 & ~r2 & ~r3 & (nb > _dot(m, m))
        live = r1 | r2 | r3 | r4
        b[r1] = -b[r1]
        a[r2], b[r2] = b[r2].copy(), a[r2].copy()
        b[r3] = p[r3]
        b[r4] = m[r4]
    return a, b, ~live


def plane(lat32, hkl, max_area):
    """One plane of one cell: dict(vec [6], area, mult, status)."""
    out = dict(vec=np.zeros(6), area=0.0, mult=0, status=BAD_CELL)
    L = np.asarray(lat32, np.float32).reshape(9).astype(np.float64)
    if not np.isfinite(L).all() or max(abs(int(v)) for v in hkl) > MAX_MILLER:
        return out
    det = (L[0] * (L[4] * L[8] - L[5] * L[7]) - L[1] * (L[3] * L[8] - L[5] * L[6])) + L[2] * (L[3] * L[7] - L[4] * L[6])
    if not (abs(det) > 0.0) or not np.isfinite(det):
        return out
    u, v = basis([int(x) for x in hkl])
    cart = lambda w: np.array([(np.float64(w[0]) * L[c] + np.float64(w[1]) * L[3 + c]) + np.float64(w[2]) * L[6 + c] for c in range(3)])
    a, b, ended = reduce_pairs(cart(u), cart(v))
    a, b = a[0], b[0]
    c = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    A = np.sqrt(_dot(c, c))
    if not (A > 0.0) or not np.isfinite(A):
        return out
    q = np.float64(max_area) / A
    capped = not (q < MAX_MULT + 1)
    return dict(vec=np.concatenate([a, b]), area=float(A), mult=MAX_MULT if capped else int(math.floor(q)),
                status=REDUCE_CAP if not ended[0] else MULT_CAP if capped else OK)


def table(vec, mult):
    """(entries [OFFSET[mult + 1], 3] = (|a'|, |b'|, theta'), ended [same] per entry) of a plane's superlattices n = 1 .. mult."""
    hs = np.array([h for n in range(1, mult + 1) for h in hnfs(n)], np.float64).reshape(-1, 3)
    a, b = np.asarray(vec[:3], np.float64), np.asarray(vec[3:], np.float64)
    x = hs[:, 0:1] * a[None] + hs[:, 1:2] * b[None]
    y = hs[:, 2:3] * b[None]
    x, y, ended = reduce_pairs(x, y)
    la, lb = np.sqrt(_dot(x, x)), np.sqrt(_dot(y, y))
    with np.errstate(invalid="ignore", divide="ignore"):
        cs = np.clip(_dot(x, y) / (la * lb), -1.0, 1.0)
    return Table(np.stack([la, lb, np.arccos(cs)], 1).reshape(-1, 3), ended, x, y)


class Table(tuple):
    """(entries, ended) of a plane, with the reduced vectors x, y [E, 3] the entries were computed from."""

    def __new__(cls, entries, ended, x=None, y=None):
        self = super().__new__(cls, (entries, ended))
        self.x, self.y = (np.zeros((0, 3)), np.zeros((0, 3))) if x is None else (x, y)
        return self


NO_TABLE = Table(np.zeros((0, 3)), np.zeros(0, bool))


class Margin:
    """The smallest |quantity - tolerance| over the decisions taken."""

    def __init__(self):
        self.value = math.inf

    def see(self, quantity, tol):
        q = np.abs(np.abs(np.asarray(quantity, np.float64)) - tol)
        if q.size:
            self.value = min(self.value, float(np.nanmin(q)))


EMPTY_D = [math.inf, math.nan, math.nan, math.nan]
EMPTY_I = [-1] + [0] * 8


def _match_rows(key, fplane, ftab, fA, stab):
    if key is None:
        return list(EMPTY_D), list(EMPTY_I)
    nf, h, ns, g = key
    f, s = ftab[OFFSET[nf] + h], stab[OFFSET[ns] + g]
    e = s / f - 1.0
    return [float(np.float64(nf) * np.float64(fA)), float(e[0]), float(e[1]), float(e[2])], [fplane, nf, ns, *hnfs(nf)[h], *hnfs(ns)[g]]


def search_item(fpl, ftab, fended, spl, stab, fplane, p, count, margin):
    """One (film plane, substrate plane) item: (row_d [10], row_i [20], n_matches)."""
    if fpl["status"] == BAD_CELL or spl["status"] == BAD_CELL:
        return EMPTY_D + [math.inf] + EMPTY_D + [0.0], [BAD_CELL] + EMPTY_I + EMPTY_I + [0], 0 if count else -1
    lowest, best, n, cap = None, None, 0, False
    ratio = np.float64(fpl["area"]) / np.float64(spl["area"])
    for nf in range(1, fpl["mult"] + 1):
        F = ftab[OFFSET[nf]:OFFSET[nf + 1]]
        cap = cap or not fended[OFFSET[nf]:OFFSET[nf + 1]].all()
        found = []
        for ns in range(1, spl["mult"] + 1):
            d = abs(ratio - np.float64(ns) / np.float64(nf))
            margin.see(d, p["max_area_ratio_tol"])
            if not d < p["max_area_ratio_tol"]:
                continue
            S = stab[OFFSET[ns]:OFFSET[ns + 1]]
            e = S[None, :, :] / F[:, None, :] - 1.0
            margin.see(e[..., :2], p["max_length_tol"])
            margin.see(e[..., 2], p["max_angle_tol"])
            ok = (np.abs(e[..., 0]) <= p["max_length_tol"]) & (np.abs(e[..., 1]) <= p["max_length_tol"]) & (np.abs(e[..., 2]) <= p["max_angle_tol"])
            if not ok.any():
                continue
            hh, gg = np.nonzero(ok)   # row-major: ascending (h, g)
            found.append((int(hh[0]), ns, int(gg[0])))
            if count:
                n += int(ok.sum())
                strain = np.abs(e[hh, gg]).max(1)
                k = int(np.flatnonzero(strain == strain.min())[0])   # of equal strains the lowest (h, g)
                cand = (float(strain[k]), (nf, int(hh[k]), ns, int(gg[k])))
                if best is None or cand < best:
                    best = cand
        if found and lowest is None:
            h, ns, g = min(found)
            lowest = (nf, h, ns, g)
            if not count:
                break
    flag = max(fpl["status"], spl["status"], REDUCE_CAP if cap else OK)
    d0, i0 = _match_rows(lowest, fplane, ftab, fpl["area"], stab)
    d1, i1 = _match_rows(best[1] if best else None, fplane, ftab, fpl["area"], stab)
    return d0 + [best[0] if best else math.inf] + d1 + [0.0], [flag] + i0 + i1 + [0], n if count else -1


def _row_status(flag, found):
    return flag if flag != OK else OK if found else NO_MATCH


def analyze(film_lats, film_hkls, bank, params=None, count=False):
    """The device pipeline.  film_lats [B, 9] float32; film_hkls [Pf, 3]; bank: a list of (lat [9] float32, hkls [k, 3]) per substrate.
    A dict of the device's arrays (f_* and s_* of the planes, s_table, res_d, res_i, res_n, mcia, mcia_plane, mcia_status) and `margin`."""
    p = dict(DEFAULTS, **(params or {}))
    film_lats = np.asarray(film_lats, np.float32).reshape(-1, 9)
    B, Pf = len(film_lats), len(film_hkls)
    fpl = [[plane(film_lats[b], hkl, p["max_area"]) for hkl in film_hkls] for b in range(B)]
    spl, sub_off = [], [0]
    for lat, hkls in bank:
        spl += [plane(lat, hkl, p["max_area"]) for hkl in hkls]
        sub_off.append(len(spl))
    Ps, S = len(spl), len(bank)
    stabs = []
    s_table = np.zeros((Ps, TABLE, 3))
    for q in spl:
        if q["status"] == BAD_CELL:
            stabs.append(NO_TABLE)
            continue
        stabs.append(table(q["vec"], q["mult"]))
        if not stabs[-1][1].all():
            q["status"] = max(q["status"], REDUCE_CAP)
    for k, (t, _) in enumerate(stabs):
        s_table[k, :len(t)] = t
    margin = Margin()
    res_d, res_i, res_n = np.zeros((B, Ps, ROW_D)), np.zeros((B, Ps, ROW_I), np.int32), np.zeros((B, Ps), np.int64)
    f_tabs = []
    for b in range(B):
        ftabs = [table(q["vec"], q["mult"]) if q["status"] != BAD_CELL else NO_TABLE for q in fpl[b]]
        f_tabs += ftabs
        for sp in range(Ps):
            items = [search_item(fpl[b][fp], ftabs[fp][0], ftabs[fp][1], spl[sp], stabs[sp][0], fp, p, count, margin) for fp in range(Pf)]
            flag, low, ls, area, strain, n = OK, -1, -1, math.inf, math.inf, 0
            for fp, (d, r, k) in enumerate(items):
                flag = max(flag, r[0])
                if d[0] < area:
                    area, low = d[0], fp
                if d[4] < strain:
                    strain, ls = d[4], fp
                n += k
            dl, rl = items[max(low, 0)][:2]
            ds, rs = items[max(ls, 0)][:2]
            res_d[b, sp] = dl[:4] + ds[4:]
            res_i[b, sp] = [_row_status(flag, low >= 0)] + rl[1:10] + rs[10:]
            res_n[b, sp] = n if count else -1
    mcia, mcia_plane, mcia_status = np.full((B, S), math.inf), np.full((B, S), -1, np.int32), np.zeros((B, S), np.int32)
    for b in range(B):
        for s in range(S):
            flag = OK
            for sp in range(sub_off[s], sub_off[s + 1]):
                st = int(res_i[b, sp, 0])
                flag = max(flag, st if st >= MULT_CAP else OK)
                if res_d[b, sp, 0] < mcia[b, s]:
                    mcia[b, s], mcia_plane[b, s] = res_d[b, sp, 0], sp
            mcia_status[b, s] = _row_status(flag, mcia_plane[b, s] >= 0)
    flat = [q for row in fpl for q in row]
    pack = lambda qs, k, dt: np.array([q[k] for q in qs], dt).reshape(len(qs), *np.shape(qs[0][k])) if qs else np.zeros(0, dt)
    return dict(f_vec=pack(flat, "vec", np.float64), f_area=pack(flat, "area", np.float64), f_mult=pack(flat, "mult", np.int32), f_status=pack(flat, "status", np.int32),
                s_vec=pack(spl, "vec", np.float64), s_area=pack(spl, "area", np.float64), s_mult=pack(spl, "mult", np.int32), s_status=pack(spl, "status", np.int32),
                s_table=s_table, sub_off=np.array(sub_off, np.int32), res_d=res_d, res_i=res_i, res_n=res_n, mcia=mcia, mcia_plane=mcia_plane,
                mcia_status=mcia_status, margin=margin.value, f_tabs=f_tabs, s_tabs=stabs)


# ---- the restatement's own deviation from a higher-precision evaluation of the same formulas ------------------------------------------------------
def _precise(tab, span=None):
    """(|a|, |b|, theta) of every entry of a Table from its reduced float64 vectors: mpmath at 200 bits (sums and products of doubles are
    then exact) if present, else numpy.longdouble with arctan2.  An object array [E, 3]."""
    try:
        import mpmath as mp
    except ImportError:
        mp = None
    lo, hi = (0, len(tab.x)) if span is None else span
    out = np.empty((len(tab.x), 3), object)
    for k in range(lo, hi):
        x, y = tab.x[k], tab.y[k]
        if mp is not None:
            with mp.workprec(200):
                xs, ys = [mp.mpf(float(v)) for v in x], [mp.mpf(float(v)) for v in y]
                la, lb = mp.sqrt(sum(v * v for v in xs)), mp.sqrt(sum(v * v for v in ys))
                cs = sum(a * b for a, b in zip(xs, ys)) / (la * lb)
                out[k] = [la, lb, mp.acos(max(-1, min(1, cs)))]
        else:
            xs, ys = np.asarray(x, np.longdouble), np.asarray(y, np.longdouble)
            la, lb = np.sqrt((xs * xs).sum()), np.sqrt((ys * ys).sum())
            cs = min(np.longdouble(1), max(np.longdouble(-1), (xs * ys).sum() / (la * lb)))
            out[k] = [la, lb, np.arctan2(np.sqrt((1 - cs) * (1 + cs)), cs)]
    return out


def deviation(ref):
    """dict(theta, strain): the largest |float64 - precise| of theta over every substrate table entry of an `analyze` result (the film
    tables are no output of the device), and of the three strains
    over every (film HNF, substrate HNF) pair of the (n_f, n_s) blocks its reported matches lie in."""
    B, Ps = ref["res_i"].shape[:2]
    Pf = len(ref["f_tabs"]) // max(B, 1)
    hp = {}

    def precise(kind, k, span=None):
        if (kind, k, span) not in hp:
            hp[kind, k, span] = _precise(ref[kind + "_tabs"][k], span)
        return hp[kind, k, span]

    dev_t = 0.0
    for k, tab in enumerate(ref["s_tabs"]):
        if len(tab[0]):
            dev_t = max(dev_t, max(abs(float(p - float(v))) for p, v in zip(precise("s", k)[:, 2], tab[0][:, 2])))
    dev_s = 0.0
    for b in range(B):
        for sp in range(Ps):
            for which in (0, 1):
                r = [int(v) for v in ref["res_i"][b, sp, 1 + 9 * which:10 + 9 * which]]
                if r[0] < 0:
                    continue
                fk, nf, ns = b * Pf + r[0], r[1], r[2]
                F, S = ref["f_tabs"][fk][0][OFFSET[nf]:OFFSET[nf + 1]], ref["s_tabs"][sp][0][OFFSET[ns]:OFFSET[ns + 1]]
                Fp, Sp = precise("f", fk, (OFFSET[nf], OFFSET[nf + 1]))[OFFSET[nf]:OFFSET[nf + 1]], precise("s", sp)[OFFSET[ns]:OFFSET[ns + 1]]
                e = S[None] / F[:, None] - 1.0
                for h in range(len(F)):
                    for g in range(len(S)):
                        dev_s = max(dev_s, max(abs(float(Sp[g, c] / Fp[h, c] - 1 - float(e[h, g, c]))) for c in range(3)))
    return dict(theta=dev_t, strain=dev_s)


# ---- the independent brute force -----------------------------------------------------------------------------------------------------------------
def _reduce_rec(a, b, depth=0):
    """reduce_vectors as a recursion on Python floats; (a, b) or None past 64 applications."""
    dot = lambda x, y: (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]
    if depth == REDUCE_ITERS:
        return None
    if dot(a, b) < 0.0:
        return _reduce_rec(a, [-v for v in b], depth + 1)
    if dot(a, a) > dot(b, b):
        return _reduce_rec(b, a, depth + 1)
    plus = [y + x for x, y in zip(a, b)]
    if dot(b, b) > dot(plus, plus):
        return _reduce_rec(a, plus, depth + 1)
    minus = [y - x for x, y in zip(a, b)]
    if dot(b, b) > dot(minus, minus):
        return _reduce_rec(a, minus, depth + 1)
    return a, b


def _brute_plane(lat32, hkl, max_area):
    """(area, [(n, idx, |a|, |b|, theta)] over every superlattice of the plane) or None for a cell without planes."""
    L = [[float(np.float32(v)) for v in row] for row in np.asarray(lat32, np.float32).reshape(3, 3)]
    if not all(math.isfinite(v) for row in L for v in row):
        return None
    u, v = basis(hkl)
    cart = lambda w: [(w[0] * L[0][c] + w[1] * L[1][c]) + w[2] * L[2][c] for c in range(3)]
    red = _reduce_rec(cart(u), cart(v))
    assert red is not None
    a, b = red
    cr = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    A = math.sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2])
    if not A > 0.0:
        return None
    out = []
    for n in range(1, min(MAX_MULT, int(math.floor(max_area / A))) + 1):
        idx = 0
        for i in range(1, n + 1):
            if n % i:
                continue
            for j in range(n // i):
                red = _reduce_rec([i * x + j * y for x, y in zip(a, b)], [(n // i) * y for y in b])
                assert red is not None
                x, y = red
                la, lb = math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]), math.sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2])
                cs = ((x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]) / (la * lb)
                out.append((n, idx, la, lb, math.acos(max(-1.0, min(1.0, cs)))))
                idx += 1
    return A, out


def brute(film_lat, film_hkls, sub_lat, sub_hkl, params=None):
    """Every match of one film on one substrate plane, by plain loops without an early exit: dict(area, key = (film plane, n_f, film HNF
    index, n_s, substrate HNF index) of the lowest match, n_matches, ls_key and ls_strain of the least strained one); area = inf and the
    keys None where nothing matches."""
    p = dict(DEFAULTS, **(params or {}))
    sub = _brute_plane(sub_lat, sub_hkl, p["max_area"])
    matches = []
    for fp, hkl in enumerate(film_hkls):
        film = _brute_plane(film_lat, hkl, p["max_area"])
        if film is None or sub is None:
            continue
        (Af, fs), (As, ss) = film, sub
        S = np.array([e[2:] for e in ss]).reshape(-1, 3)
        sn = np.array([e[0] for e in ss])
        for nf, h, la, lb, th in fs:
            adm = np.abs(Af / As - sn / nf) < p["max_area_ratio_tol"]
            e = S / np.array([la, lb, th]) - 1.0
            ok = adm & (np.abs(e[:, 0]) <= p["max_length_tol"]) & (np.abs(e[:, 1]) <= p["max_length_tol"]) & (np.abs(e[:, 2]) <= p["max_angle_tol"])
            for k in np.flatnonzero(ok):
                matches.append((nf * Af, float(np.abs(e[k]).max()), (fp, nf, h, int(ss[k][0]), int(ss[k][1]))))
    if not matches:
        return dict(area=math.inf, key=None, n_matches=0, ls_key=None, ls_strain=math.inf)
    low = min(matches, key=lambda m: (m[0], m[2]))
    ls = min(matches, key=lambda m: (m[1], m[2]))
    return dict(area=low[0], key=low[2], n_matches=len(matches), ls_key=ls[2], ls_strain=ls[1])


def row_key(row_i, which=0):
    """(film plane, n_f, film HNF index, n_s, substrate HNF index) of a result row's lowest (which = 0) or least strained (1) match."""
    r = [int(v) for v in row_i[1 + 9 * which:10 + 9 * which]]
    if r[0] < 0:
        return None
    return (r[0], r[1], hnfs(r[1]).index(tuple(r[3:6])), r[2], hnfs(r[2]).index(tuple(r[6:9])))


# ---- the files of scripts/zsl_host_check.cpp ------------------------------------------------------------------------------------------------------
def write_case(path, film_lats, film_hkls, bank, params, count):
    """int32 B, Pf, Ps, S, count; float64 max_area, max_area_ratio_tol, max_length_tol, max_angle_tol; film lat [B][9] f32; film hkl
    [Pf][3] i32; substrate lat [S][9] f32; plane hkl [Ps][3], cell_of [Ps], sub_off [S + 1] i32."""
    p = dict(DEFAULTS, **(params or {}))
    film_lats = np.asarray(film_lats, np.float32).reshape(-1, 9)
    hk = np.asarray(film_hkls, np.int32).reshape(-1, 3)
    s_lat = np.array([np.asarray(l, np.float32).reshape(9) for l, _ in bank], np.float32).reshape(-1, 9)
    s_hkl = np.array([h for _, hs in bank for h in hs], np.int32).reshape(-1, 3)
    cell_of = np.array([s for s, (_, hs) in enumerate(bank) for _ in hs], np.int32)
    sub_off = np.cumsum([0] + [len(hs) for _, hs in bank]).astype(np.int32)
    with open(path, "wb") as f:
        f.write(struct.pack("<5i4d", len(film_lats), len(hk), len(s_hkl), len(bank), int(count), p["max_area"], p["max_area_ratio_tol"], p["max_length_tol"],
                            p["max_angle_tol"]))
        for arr in (film_lats, hk, s_lat, s_hkl, cell_of, sub_off):
            f.write(np.ascontiguousarray(arr).tobytes())


def read_out(path, B, Pf, Ps, S):
    """The arrays of `analyze`, as the host check wrote them."""
    raw = open(path, "rb").read()
    at = 0

    def take(shape, dt):
        nonlocal at
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        arr = np.frombuffer(raw[at:at + n], dt).reshape(shape).copy()
        at += n
        return arr

    out = {}
    for pre, T in (("f", B * Pf), ("s", Ps)):
        out[pre + "_vec"], out[pre + "_area"], out[pre + "_mult"], out[pre + "_status"] = take((T, 6), np.float64), take((T,), np.float64), take((T,), np.int32), take((T,), np.int32)
    out["s_table"] = take((Ps, TABLE, 3), np.float64)
    out["res_d"], out["res_i"], out["res_n"] = take((B, Ps, ROW_D), np.float64), take((B, Ps, ROW_I), np.int32), take((B, Ps), np.int64)
    out["mcia"], out["mcia_plane"], out["mcia_status"] = take((B, S), np.float64), take((B, S), np.int32), take((B, S), np.int32)
    assert at == len(raw), (at, len(raw))
    return out
