"""The conventional cell of DESIGN 53 restated in plain Python integers and float64, operation for operation, on top of tests/sm_ref64.py and
tests/sym_ref64.py: the executable form of csrc/sym_conv.h, and the reference every output of mi_sym_conventional is held to bit for bit.
Also the chain primitive -> conventional the host module runs, and the certificate: a check of a returned cell from the input alone in
numpy's own operations.  A search asserts that no candidate the symmetry does not carry onto the winner lies within MARGIN of the winner's
squared length (margin=False switches that off); `box` widens the search for the box-margin test."""
import itertools
import math

import numpy as np

from tests import sm_ref64 as R
from tests import sym_ref64 as S

CONV_FAIL = 512
NINFO, BOX, MAX_MULT, Q_MAX, M_MAX, T_MAX = 8, 2, 4, 1 << 14, 8, 512
NONE, P_, A_, B_, C_, I_, F_, R_ = range(8)
CENTRING = ("", "P", "A", "B", "C", "I", "F", "R")
BRAVAIS = ("", "aP", "mP", "mS", "oP", "oS", "oI", "oF", "tP", "tI", "hR", "hP", "cP", "cI", "cF")
INFO = ("bravais", "centring", "mult", "crystal_system", "n_axes", "max_m", "zero", "status")
MARGIN = 1e-9
IDENT = [1, 0, 0, 0, 1, 0, 0, 0, 1]


def imul(A, B):
    return [A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j] for i in range(3) for j in range(3)]


def row_mul(k, A):
    return [k[0] * A[c] + k[1] * A[3 + c] + k[2] * A[6 + c] for c in range(3)]


def proper(W):
    d = R.idet3(W)
    return [d * int(v) for v in W]


def order_of(P):
    M = list(P)
    for n in range(1, 7):
        if M == IDENT:
            return 0 if n == 5 else n
        M = imul(M, P)
        if any(abs(v) > Q_MAX for v in M):
            return 0
    return 0


def axis_sum(P, n):
    Ssum, M = [0] * 9, list(IDENT)
    for _ in range(n):
        Ssum = [a + b for a, b in zip(Ssum, M)]
        M = imul(M, P)
    return Ssum


def axis_of(Ssum):
    for i in range(3):
        r = Ssum[3 * i:3 * i + 3]
        if any(r):
            g = math.gcd(math.gcd(abs(r[0]), abs(r[1])), abs(r[2]))
            lead = next(v for v in r if v != 0)
            s = -g if lead < 0 else g
            return [v // s for v in r]   # (exact: s divides every entry)
    return None


def classify(W):
    P = proper(W)
    n = order_of(P)
    k = [0, 0, 0]
    if n >= 2:
        k = axis_of(axis_sum(P, n))
        if k is None:
            n, k = 0, [0, 0, 0]
    return n, k


def collect(rot):
    """The distinct axes by order and the first operation of each order, over the rotation parts that differ from the one before."""
    ax = {"ax2": [], "ax3": [], "ax4": [], "first2": -1, "first3": -1, "first4": -1, "first6": -1, "bad": False}
    caps = {2: 9, 3: 4, 4: 3}
    for i, W in enumerate(rot):
        W = [int(v) for v in W]
        if i > 0 and W == [int(v) for v in rot[i - 1]]:
            continue
        n, k = classify(W)
        if n == 1:
            continue
        if n == 0:
            ax["bad"] = True
        if n in (2, 3, 4):
            if ax["first%d" % n] < 0:
                ax["first%d" % n] = i
            lst = ax["ax%d" % n]
            if k not in lst:
                if len(lst) >= caps[n]:
                    ax["bad"] = True
                else:
                    lst.append(k)
        if n == 6 and ax["first6"] < 0:
            ax["first6"] = i
    return ax


def gdot(G, a, b):
    a0, a1, a2 = float(a[0]), float(a[1]), float(a[2])
    v0, v1, v2 = (a0 * G[0] + a1 * G[3]) + a2 * G[6], (a0 * G[1] + a1 * G[4]) + a2 * G[7], (a0 * G[2] + a1 * G[5]) + a2 * G[8]
    return (v0 * float(b[0]) + v1 * float(b[1])) + v2 * float(b[2])


def box_k(p, box):
    side = 2 * box + 1
    return [box - p // (side * side), box - (p // side) % side, box - p % side]


def parallel(a, b):
    return a[1] * b[2] - a[2] * b[1] == 0 and a[2] * b[0] - a[0] * b[2] == 0 and a[0] * b[1] - a[1] * b[0] == 0


def search(Ssum, excl, G, box, images=None):
    """The point of the box with the smallest (k G k^T, index) among the non-zero k with k S = 0 that are not parallel to excl, or None.
    images(k): the vectors the symmetry carries k onto -- with it, every other candidate within MARGIN of the winner must be one of them."""
    best, bp, cands = R.INF, None, []
    for p in range((2 * box + 1) ** 3):
        k = box_k(p, box)
        if not any(k) or any(row_mul(k, Ssum)) or (excl is not None and parallel(k, excl)):
            continue
        l2 = gdot(G, k, k)
        cands.append((l2, k))
        if l2 < best:   # (ascending p: of equal lengths the lower index stays)
            best, bp = l2, p
    if bp is None:
        return None
    k = box_k(bp, box)
    if images is not None:
        same = images(k)
        for l2, c in cands:
            assert abs(l2 - best) > MARGIN or tuple(c) in same, ("search", k, c, l2, best)
    return k


def basis(system, ax, rot, G, box=BOX, margin=True):
    """(ok, M, n_axes)."""
    M = list(IDENT)
    if ax["bad"]:
        return False, M, 0
    parts = []
    for W in rot:
        Pm = proper([int(v) for v in W])
        if Pm not in parts:
            parts.append(Pm)

    def images(k):
        out = set()
        for Pm in parts:
            r = row_mul(k, Pm)
            out.add(tuple(r)), out.add(tuple(-v for v in r))
        return out

    if system == 1:
        return True, M, 0
    if system == 2:
        if len(ax["ax2"]) != 1 or ax["first2"] < 0:
            return False, M, len(ax["ax2"])
        Ssum = axis_sum(proper(rot[ax["first2"]]), 2)
        a = search(Ssum, None, G, box)   # (a tie of a with the vector that becomes c only exchanges their names)
        if a is None:
            return False, M, 1
        c = search(Ssum, a, G, box, images if margin else None)
        if c is None:
            return False, M, 1
        if gdot(G, a, c) > 0.0:
            c = [-v for v in c]
        return True, a + ax["ax2"][0] + c, 1
    if system == 3:
        if len(ax["ax2"]) != 3:
            return False, M, len(ax["ax2"])
        r = [list(k) for k in ax["ax2"]]
        l2 = [gdot(G, k, k) for k in r]
        for i, j in ((0, 1), (1, 2), (0, 1)):   # (of equal lengths the earlier axis first: the order names the axes and decides nothing else)
            if l2[j] < l2[i]:
                r[i], r[j], l2[i], l2[j] = r[j], r[i], l2[j], l2[i]
        return True, r[0] + r[1] + r[2], 3
    if system in (4, 5, 6):
        if system == 4:
            n_axes, order = len(ax["ax4"]), 4
            if n_axes != 1 or ax["first4"] < 0:
                return False, M, n_axes
            Pm = proper(rot[ax["first4"]])
        else:
            n_axes, order = len(ax["ax3"]), 3
            if n_axes > 1:
                return False, M, n_axes
            if ax["first3"] >= 0:
                Pm = proper(rot[ax["first3"]])
            else:
                if ax["first6"] < 0:
                    return False, M, n_axes
                P6 = proper(rot[ax["first6"]])
                Pm, n_axes = imul(P6, P6), 1
        Ssum = axis_sum(Pm, order)
        c = axis_of(Ssum)
        if c is None:
            return False, M, n_axes
        a = search(Ssum, None, G, box, images if margin else None)
        if a is None:
            return False, M, n_axes
        return True, a + row_mul(a, Pm) + c, n_axes
    if system == 7:
        lst = ax["ax4"] if ax["ax4"] else ax["ax2"]
        if len(lst) != 3:
            return False, M, len(lst)
        r = sorted((list(k) for k in lst), reverse=True)
        return True, r[0] + r[1] + r[2], 3
    return False, M, 0


def orient(system, M):
    d = R.idet3(M)
    if d < 0:
        r = 3 if system == 2 else 6   # (monoclinic: b, whose sign is free; c's is taken by beta >= 90 degrees)
        M[r:r + 3] = [-v for v in M[r:r + 3]]
        d = -d
    return d


def centring_vectors(M, d):
    A = R.iadj3(M)
    vs = set()
    for k in itertools.product(range(d), repeat=3):
        vs.add(tuple(v % d for v in row_mul(list(k), A)))
    return sorted(vs)


def centring_name(d, vs):
    """(letter index, reverse)."""
    if len(vs) != d or vs[0] != (0, 0, 0):
        return NONE, False
    table = {(): P_, ((1, 1, 1),): I_, ((1, 1, 0),): C_, ((1, 0, 1),): B_, ((0, 1, 1),): A_, ((0, 2, 2), (2, 0, 2), (2, 2, 0)): F_}
    rest = tuple(vs[1:])
    if d == 3:
        return (R_, False) if rest == ((1, 2, 2), (2, 1, 1)) else ((R_, True) if rest == ((1, 2, 1), (2, 1, 2)) else (NONE, False))
    name = table.get(rest, NONE)
    if (d, name) not in ((1, P_), (2, I_), (2, C_), (2, B_), (2, A_), (4, F_)):
        return NONE, False
    return name, False


def bravais_of(system, c):
    return {1: {P_: 1}, 2: {P_: 2, A_: 3, C_: 3, I_: 3}, 3: {P_: 4, C_: 5, I_: 6, F_: 7}, 4: {P_: 8, I_: 9}, 5: {R_: 10, P_: 11}, 6: {P_: 11},
            7: {P_: 12, I_: 13, F_: 14}}.get(system, {}).get(c, 0)


def finish(system, M):
    """(bravais, M, mult, centring, vectors): bravais 0 on a failure."""
    M = list(M)
    for rnd in range(2):
        d = orient(system, M)
        if d < 1 or d > MAX_MULT:
            return 0, M, 1, NONE, []
        vs = centring_vectors(M, d)
        if len(vs) > MAX_MULT:
            return 0, M, 1, NONE, []
        name, reverse = centring_name(d, vs)
        if name == NONE:
            return 0, M, 1, NONE, []
        if rnd == 0 and system == 3 and name in (A_, B_):
            M = M[3:6] + M[6:9] + M[0:3] if name == A_ else M[0:3] + M[6:9] + M[3:6]
            continue
        if rnd == 0 and name == R_ and reverse:
            M = [-v for v in M[:6]] + M[6:]
            continue
        if reverse:
            return 0, M, 1, NONE, []
        bv = bravais_of(system, name)
        return (bv, M, d, name, vs) if bv else (0, M, 1, NONE, [])
    return 0, M, 1, NONE, []


def transform(M, T):
    if any(abs(v) > T_MAX for v in T) or any(abs(v) > M_MAX for v in M):
        return None
    return R.iadj3(imul(M, T))


def conv_frac(f32, adj, v, mult):
    f0, f1, f2 = float(f32[0]), float(f32[1]), float(f32[2])
    out = []
    for c in range(3):
        x = (f0 * float(adj[c]) + f1 * float(adj[3 + c])) + f2 * float(adj[6 + c])
        w = np.float32(R.wrap01((x + float(v[c])) / float(mult)))
        out.append(np.float32(0.0) if w >= np.float32(1.0) else w)
    return out


def conventional(P, types, frac, lat, F, fill=0, box=BOX, margin=True):
    """mi_sym_conventional: dict of conv_info [B, 8], conv_M [B, 9], conv_cvec [B, 4, 3], conv_count [B], conv_offsets [B + 1], types [4 N],
    frac [4 N, 3] float32, lat [B, 9] float32.  P: the prepared set of (types, frac, lat); F: the arrays of sym_ref64.find on it.  Rows the
    kernels do not write keep `fill`."""
    types, frac = np.asarray(types, np.int32), np.asarray(frac, np.float32).reshape(-1, 3)
    lat = np.asarray(lat, np.float32).reshape(-1, 9)
    B, N = len(lat), len(types)
    out = {"conv_info": np.full((B, NINFO), fill, np.int32), "conv_M": np.full((B, 9), fill, np.int32), "conv_cvec": np.full((B, MAX_MULT, 3), fill, np.int32),
           "conv_count": np.full(B, fill, np.int32), "types": np.full(4 * N, fill, np.int32), "frac": np.full((4 * N, 3), fill, np.float32),
           "lat": np.full((B, 9), fill, np.float32)}
    rows = []

    def fail(b, n, system, n_axes, status, cell):
        out["conv_info"][b] = [0, NONE, 1, system, n_axes, 1, 0, status]
        out["conv_M"][b], out["conv_cvec"][b], out["conv_count"][b] = IDENT, 0, n
        if cell:
            out["lat"][b] = lat[b]
        n0 = int(P["offsets"][b])
        rows.append((types[n0:n0 + n].copy(), frac[n0:n0 + n].copy()))

    for b in range(B):
        st, system, nops = int(F["info"][b][7]), int(F["info"][b][5]), int(F["info"][b][0])
        if int(P["info"][b][3]) != R.PREP_OK:
            fail(b, 0, 0, 0, st | S.NOT_PREPARED | CONV_FAIL, False)
            continue
        n, n0 = int(P["info"][b][0]), int(P["offsets"][b])
        if st != S.OK or nops < 1 or nops > S.MAX_OPS:
            fail(b, n, system, 0, st | CONV_FAIL, True)
            continue
        rot = [[int(v) for v in W] for W in F["rot"][b][:nops]]
        G = S.rigid_metric([float(x) for x in P["lat"][b]])
        ok, M, n_axes = basis(system, collect(rot), rot, G, box, margin)
        bv, M, mult, cen, vs = finish(system, M) if ok else (0, M, 1, NONE, [])
        red_ok, T, Lr = R.reduce_cell([float(v) for v in lat[b]])
        assert red_ok
        adj = transform(M, T) if bv else None
        if adj is None:
            fail(b, n, system, n_axes, st | CONV_FAIL, True)
            continue
        out["conv_info"][b] = [bv, cen, mult, system, n_axes, max(abs(v) for v in M), 0, st]
        out["conv_M"][b] = M
        out["conv_cvec"][b] = [list(v) for v in vs] + [[0, 0, 0]] * (MAX_MULT - len(vs))
        out["conv_count"][b] = mult * n
        out["lat"][b] = [np.float32((float(M[3 * i]) * Lr[c] + float(M[3 * i + 1]) * Lr[3 + c]) + float(M[3 * i + 2]) * Lr[6 + c]) for i in range(3) for c in range(3)]
        zs, fs = [], []
        for i in range(n):
            for j in range(mult):
                zs.append(types[n0 + i]), fs.append(conv_frac(frac[n0 + i], adj, vs[j], mult))
        rows.append((np.asarray(zs, np.int32), np.asarray(fs, np.float32).reshape(-1, 3)))
    off = np.concatenate([[0], np.cumsum(out["conv_count"])]).astype(np.int32)
    out["conv_offsets"] = off
    for b, (z, fr) in enumerate(rows):
        lo, hi = int(off[b]), min(int(off[b]) + len(z), 4 * N)
        if hi > lo:
            out["types"][lo:hi], out["frac"][lo:hi] = z[:hi - lo], fr[:hi - lo]
    return out


def chain(batch, symprec, cos_tol, fill=0, box=BOX, margin=True):
    """The host module's chain on a batch (offsets, types, frac, lat): prepare -> find -> primitive -> prepare -> find -> conventional, the
    second find with the first one's tolerances (the prepared units are volume per atom, which the primitive cell keeps).  Returns a dict:
    the stages under their names and the conventional arrays under "conv"."""
    off, types, frac, lat = batch
    tol = S.tolerances(np.clip(off, 0, len(types)), lat, symprec)
    P1 = R.prepare(off, types, frac, lat)
    F1 = S.find(P1, tol, cos_tol, margin=margin)
    prim = S.primitive(P1, types, frac, lat, F1, margin=margin)
    P2 = R.prepare(prim["prim_offsets"], prim["types"], prim["frac"], prim["lat"])
    F2 = S.find(P2, tol, cos_tol, fill=fill, margin=margin)
    conv = conventional(P2, prim["types"], prim["frac"], prim["lat"], F2, fill=fill, box=box, margin=margin)
    return {"tol": tol, "P1": P1, "F1": F1, "prim": prim, "P2": P2, "F2": F2, "conv": conv}


def crystal_of(conv, b):
    """(lattice [3, 3] float64, types, frac [n, 3] float64) of crystal b of conventional()'s arrays."""
    lo, hi = int(conv["conv_offsets"][b]), int(conv["conv_offsets"][b + 1])
    return conv["lat"][b].reshape(3, 3).astype(np.float64), [int(v) for v in conv["types"][lo:hi]], conv["frac"][lo:hi].astype(np.float64)


def cell_parameters(L):
    """(a, b, c, alpha, beta, gamma), degrees, of a cell [3, 3] in numpy's own operations."""
    L = np.asarray(L, np.float64).reshape(3, 3)
    ln = np.linalg.norm(L, axis=1)
    ang = [math.degrees(math.acos(max(-1.0, min(1.0, float(L[i] @ L[j] / (ln[i] * ln[j])))))) for i, j in ((1, 2), (0, 2), (0, 1))]
    return [float(v) for v in ln] + ang


# ---- the certificate: from the outputs and the input alone --------------------------------------------------------------------------------------
def metric_ok(system, centring, params, symprec, angle_tol):
    """The conventional metric meets its system's constraints: lengths within symprec, angles within angle_tol degrees."""
    a, b, c, al, be, ga = params
    eq, ang = (lambda x, y: abs(x - y) <= symprec), (lambda x, y: abs(x - y) <= angle_tol)
    if system == 1:
        return True
    if system == 2:
        return ang(al, 90) and ang(ga, 90) and be >= 90 - angle_tol
    if system == 3:
        return ang(al, 90) and ang(be, 90) and ang(ga, 90)
    if system == 4:
        return eq(a, b) and ang(al, 90) and ang(be, 90) and ang(ga, 90)
    if system in (5, 6):
        return eq(a, b) and ang(al, 90) and ang(be, 90) and ang(ga, 120)
    return eq(a, b) and eq(b, c) and ang(al, 90) and ang(be, 90) and ang(ga, 90)


def certificate(primitive, conv_crystal, M, mult, system, centring, symprec, angle_tol):
    """primitive, conv_crystal: (lattice, types, frac).  |det M| = mult; mult x n_prim atoms, all distinct; the metric meets the system's
    constraints; every conventional atom is a primitive atom plus a lattice vector of the primitive cell (same species)."""
    Lp, zp, fp = np.asarray(primitive[0], np.float64).reshape(3, 3), list(primitive[1]), np.asarray(primitive[2], np.float64).reshape(-1, 3)
    Lc, zc, fc = np.asarray(conv_crystal[0], np.float64).reshape(3, 3), list(conv_crystal[1]), np.asarray(conv_crystal[2], np.float64).reshape(-1, 3)
    assert abs(round(np.linalg.det(np.asarray(M, np.float64).reshape(3, 3)))) == mult
    assert abs(abs(np.linalg.det(Lc)) / abs(np.linalg.det(Lp)) - mult) < 1e-4 * mult
    assert len(zc) == mult * len(zp) and sorted(zc) == sorted(list(zp) * mult)
    assert metric_ok(system, centring, cell_parameters(Lc), symprec, angle_tol), cell_parameters(Lc)
    cart = fc @ Lc
    shifts = np.array(list(itertools.product((-1, 0, 1), repeat=3)), np.float64)
    for i in range(len(zc)):
        for j in range(i + 1, len(zc)):
            d = fc[i] - fc[j]
            d = d - np.round(d)
            assert np.sqrt((((d[None, :] + shifts) @ Lc) ** 2).sum(1).min()) > 1e-3, ("distinct", i, j)
    Lpinv = np.linalg.inv(Lp)
    scale = float(np.abs(Lc).max())
    for i in range(len(zc)):
        g = cart[i] @ Lpinv
        hit = False
        for a in range(len(zp)):
            if zp[a] != zc[i]:
                continue
            d = g - fp[a]
            hit = hit or float(np.abs((d - np.round(d)) @ Lp).max()) < 1e-5 * scale
        assert hit, ("atom", i)
    return True
