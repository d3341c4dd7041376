"""The energy above the convex hull (include/matinvent_hip_hull.h, matinvent_amd/csrc/hull_simplex.h) restated in numpy float64
with no device code in it, and an independent value.

  * `simplex`: the header's revised simplex, operation for operation -- every product and addition rounded separately, sums ascending from
    0.0, ties to the lowest position / the lowest k -- so that the device's bits can be compared with `np.array_equal`.  It also reports
    the smallest gap between the best and the second-best choice of every entering and leaving decision: a case whose gaps all exceed TIE
    is UNTIED, and its basis and pivot count are a function of the input alone (not of the order of the candidate list).
  * `brute`: every d-subset of at most 14 candidates solved with np.linalg.solve and filtered for l >= 0 -- no simplex in it.
  * `stage`: the staging kernel's guard and dense block of one group;  `run_call`: a whole mi_hull_above call on host arrays.
  * `certificate`: the optimality conditions of a returned basis, recomputed from the input alone.
  * `make_case`: banks of integer-ratio compositions with a non-trivial hull.
"""
import itertools

import numpy as np

MAX_ELEMS, MAX_ITERS, EPS, LDS_DOUBLES = 8, 256, 1e-12, 4096
OK, NO_TERMINAL, UNBOUNDED, ITER_CAP, BAD_QUERY = 0, 1, 2, 3, 4
FLAG_SKIPPED = 1
NO_POS = 0x7FFFFFFF
TIE = 1e-9          # a decision whose runner-up is closer than this (eV/atom, or a step length) counts as tied
U = 2.0 ** -53      # float64 unit round-off


def _duals(EB, Binv, d):
    y = np.zeros(d)
    for k in range(d):
        a = 0.0
        for j in range(d):
            a = a + EB[j] * Binv[j, k]
        y[k] = a
    return y


def _gap(values):
    """second smallest - smallest of the finite entries (inf with fewer than two)"""
    v = np.sort(np.asarray(values, np.float64)[np.isfinite(values)])
    return float(v[1] - v[0]) if len(v) > 1 else np.inf


def simplex(X, E, c, e_q=np.nan):
    """One query: X [nc][d] fractions, E [nc] energies (NaN: never priced), c [d].  Returns the outputs of the header, with the basis as
    candidate POSITIONS (`decomp_pos`), and the decision gaps `gap_enter`, `gap_leave`, `gap_terminal`."""
    c = np.asarray(c, np.float64).reshape(-1)
    d = len(c)
    X = np.asarray(X, np.float64).reshape(-1, d)
    E = np.asarray(E, np.float64).reshape(-1)
    nc = len(E)
    out = dict(e_hull=np.nan, e_above=np.nan, chempot=np.full(MAX_ELEMS, np.nan), decomp_pos=np.full(MAX_ELEMS, -1, np.int64),
               decomp_frac=np.zeros(MAX_ELEMS), iters=0, status=OK, gap_enter=np.inf, gap_leave=np.inf, gap_terminal=np.inf)
    if not (np.isfinite(c).all() and (c >= 0).all()):
        out["status"] = BAD_QUERY
        return out
    finite = np.isfinite(E)
    basis = np.zeros(d, np.int64)
    for k in range(d):
        idx = np.flatnonzero(finite & (X[:, k] == 1.0))
        if len(idx) == 0:
            out["status"] = NO_TERMINAL
            return out
        basis[k] = idx[np.argmin(E[idx])]          # (argmin: the first of equal values, the lowest position)
        out["gap_terminal"] = min(out["gap_terminal"], _gap(E[idx]))
    Binv, lam, EB = np.eye(d), c.copy(), E[basis].copy()
    y = _duals(EB, Binv, d)
    iters, status = 0, OK
    while True:
        s = np.zeros(nc)
        for k in range(d):
            s = s + y[k] * X[:, k]
        r = E - s
        mask = finite.copy()
        mask[basis] = False
        if not mask.any():
            break
        rr = np.where(mask, r, np.inf)
        j = int(np.argmin(rr))
        if rr[j] >= -EPS:
            break
        if iters >= MAX_ITERS:
            status = ITER_CAP
            break
        out["gap_enter"] = min(out["gap_enter"], _gap(rr))
        u = np.zeros(d)
        for k in range(d):
            a = 0.0
            for q in range(d):
                a = a + Binv[k, q] * X[j, q]
            u[k] = a
        row, theta, ratios = -1, np.inf, []
        for k in range(d):
            if u[k] > EPS:
                t = lam[k] / u[k]
                ratios.append(t)
                if t < theta:
                    theta, row = t, k
        if row < 0:
            status = UNBOUNDED
            break
        out["gap_leave"] = min(out["gap_leave"], _gap(ratios))
        ur = u[row]
        for q in range(d):
            Binv[row, q] = Binv[row, q] / ur
        for k in range(d):
            if k == row:
                continue
            for q in range(d):
                Binv[k, q] = Binv[k, q] - u[k] * Binv[row, q]
            v = lam[k] - theta * u[k]
            lam[k] = v if v > 0.0 else 0.0
        lam[row] = theta
        EB[row] = E[j]
        basis[row] = j
        iters += 1
        y = _duals(EB, Binv, d)
    a = 0.0
    for k in range(d):
        a = a + y[k] * c[k]
    out.update(e_hull=a, e_above=e_q - a, iters=iters, status=status)
    out["chempot"] = np.concatenate([y, np.zeros(MAX_ELEMS - d)])
    out["decomp_pos"][:d] = basis
    out["decomp_frac"][:d] = lam
    return out


def untied(res):
    return min(res["gap_enter"], res["gap_leave"], res["gap_terminal"]) > TIE


def brute(X, E, c):
    """min l . E over every d-subset B of the finite candidates with B l = c solvable and l >= 0 (at most 14 candidates)."""
    c = np.asarray(c, np.float64)
    d = len(c)
    X = np.asarray(X, np.float64).reshape(-1, d)
    E = np.asarray(E, np.float64)
    idx = np.flatnonzero(np.isfinite(E))
    assert len(idx) <= 14, "brute: at most 14 candidates"
    best = np.inf
    for sub in itertools.combinations(idx, d):
        B = X[list(sub)].T
        if abs(np.linalg.det(B)) < 1e-9:
            continue
        lam = np.linalg.solve(B, c)
        if (lam >= -1e-12).all():
            best = min(best, float(np.clip(lam, 0, None) @ E[list(sub)]))
    return best


# ---- the staging kernel and a whole call ------------------------------------------------------------------------------------------------
def stage(bank, gZ, cand):
    """The dense block of one group: (X [nc][d], E [nc], rows [nc], skipped).  `bank`: dict(nelem, Z, frac, energy)."""
    gZ = [int(z) for z in gZ]
    d, nc, M = len(gZ), len(cand), len(bank["nelem"])
    X, E, rows, skipped = np.zeros((nc, d)), np.full(nc, np.nan), np.full(nc, -1, np.int64), False
    for i, idx in enumerate(cand):
        idx = int(idx)
        ok = 0 <= idx < M
        if ok:
            n = int(bank["nelem"][idx])
            ok = 1 <= n <= MAX_ELEMS
        if ok:
            f = np.zeros(d)
            for a in range(n):
                z, v = int(bank["Z"][idx, a]), float(bank["frac"][idx, a])
                if z in gZ and np.isfinite(v):
                    f[gZ.index(z)] = v
                else:
                    ok = False
        if ok:
            X[i], E[i], rows[i] = f, bank["energy"][idx], idx
        else:
            skipped = True
    return X, E, rows, skipped


def group_ok(gZ, d):
    return 1 <= d <= MAX_ELEMS and all(gZ[k] > gZ[k - 1] for k in range(1, d))


def empty_outputs(Q):
    return dict(e_hull=np.full(Q, np.nan), e_above=np.full(Q, np.nan), chempot=np.full((Q, MAX_ELEMS), np.nan), decomp_frac=np.zeros((Q, MAX_ELEMS)),
                decomp_idx=np.full((Q, MAX_ELEMS), -1, np.int64), iters=np.zeros(Q, np.int64), status=np.full(Q, -1, np.int64), flags=np.zeros(Q, np.int64))


def run_call(bank, groups, query_c, query_e, gaps=None):
    """mi_hull_above on host arrays: `groups` = dict(grp_nelem, grp_Z [G][8], grp_q_off, q_idx, grp_c_off, c_idx).  Rows of queries that no
    admissible group owns keep the pre-fill (NaN, status -1).  `gaps`: a list that receives (query row, simplex result)."""
    Q = len(query_e)
    out = empty_outputs(Q)
    G = len(groups["grp_nelem"])
    nnz_q, nnz_c = len(groups["q_idx"]), len(groups["c_idx"])
    for g in range(G):
        d = int(groups["grp_nelem"][g])
        gZ = [int(z) for z in groups["grp_Z"][g][:max(0, min(d, MAX_ELEMS))]]
        q0, q1, c0, c1 = (int(groups[k][g + o]) for k in ("grp_q_off", "grp_c_off") for o in (0, 1))
        if not (group_ok(gZ, d) and 0 <= q0 <= q1 <= nnz_q and 0 <= c0 <= c1 <= nnz_c):
            continue
        X, E, rows, skipped = stage(bank, gZ, groups["c_idx"][c0:c1])
        for q in groups["q_idx"][q0:q1]:
            q = int(q)
            if not 0 <= q < Q:
                continue
            res = simplex(X, E, query_c[q][:d], query_e[q])
            if gaps is not None:
                gaps.append((q, res))
            out["status"][q], out["iters"][q], out["flags"][q] = res["status"], res["iters"], FLAG_SKIPPED if skipped else 0
            out["e_hull"][q], out["e_above"][q], out["chempot"][q], out["decomp_frac"][q] = res["e_hull"], res["e_above"], res["chempot"], res["decomp_frac"]
            live = res["decomp_pos"] >= 0
            out["decomp_idx"][q] = -1
            out["decomp_idx"][q][live] = rows[res["decomp_pos"][live]]
    return out


# ---- the optimality certificate ------------------------------------------------------------------------------------------------------------
def certificate(X, E, c, basis_pos, lam, e_hull):
    """From the returned basis alone: y by np.linalg.solve, then the residuals of the three conditions.  Returns dict(primal = max |B l - c|,
    lam_min, dual = min over the finite candidates of E_i - y . x_i, value = |e_hull - y . c|, y)."""
    c = np.asarray(c, np.float64)
    d = len(c)
    B = np.asarray(X, np.float64)[np.asarray(basis_pos[:d], np.int64)].T          # columns x_i
    EB = np.asarray(E, np.float64)[np.asarray(basis_pos[:d], np.int64)]
    y = np.linalg.solve(B.T, EB)
    fin = np.isfinite(E)
    red = np.asarray(E)[fin] - np.asarray(X)[fin] @ y
    return dict(primal=float(np.abs(B @ np.asarray(lam[:d]) - c).max()), lam_min=float(np.min(lam[:d])), dual=float(red.min()),
                value=float(abs(e_hull - y @ c)), y=y, cond=float(np.linalg.cond(B)))


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def make_case(d, nc, seed, nq=1, on_bank=False, elems=None, nan_frac=0.0, max_count=6):
    """A bank of nc rows over d elements (the first d rows are the terminals, in a shuffled order of the list) with integer-ratio
    compositions and energies E = x . mu - depth (1 - sum x^2) w + noise, which gives a hull with several vertices; nq queries with
    integer-ratio compositions of full support (on_bank: the composition of a full-support bank row, where there is one).  Returns
    dict(gZ, bank = dict(nelem, Z, frac, energy), cand (a permutation of the rows), query_c [nq][8], query_e [nq])."""
    assert nc >= d
    rng = np.random.default_rng(seed)
    gZ = sorted(int(z) for z in (elems if elems is not None else rng.choice(np.arange(1, 95), d, replace=False)))
    mu = rng.uniform(-2.0, 0.0, d)
    counts = np.zeros((nc, d), np.int64)
    counts[:d] = np.eye(d, dtype=np.int64)
    for i in range(d, nc):
        while not counts[i].any():
            k = int(rng.integers(1, d + 1))
            on = rng.choice(d, k, replace=False)
            counts[i, on] = rng.integers(1, max_count + 1, k)
    frac = counts / counts.sum(1, keepdims=True)
    energy = frac @ mu - 0.8 * (1.0 - (frac ** 2).sum(1)) * rng.uniform(0.0, 1.0, nc) + 0.05 * rng.standard_normal(nc)
    if nan_frac > 0:
        energy[d:][rng.random(nc - d) < nan_frac] = np.nan
    nelem = (counts > 0).sum(1).astype(np.int32)
    Z, F = np.zeros((nc, MAX_ELEMS), np.int32), np.zeros((nc, MAX_ELEMS))
    for i in range(nc):
        on = np.flatnonzero(counts[i])
        Z[i, :len(on)], F[i, :len(on)] = np.asarray(gZ)[on], frac[i, on]
    qc, qe = np.zeros((nq, MAX_ELEMS)), np.zeros(nq)
    full = np.flatnonzero((counts > 0).all(1))
    for q in range(nq):
        if on_bank and len(full):
            x = frac[full[int(rng.integers(len(full)))]]
        else:
            n = rng.integers(1, max_count + 2, d)
            x = n / n.sum()
        qc[q, :d] = x
        qe[q] = x @ mu - 0.3 + 0.2 * rng.standard_normal()
    return dict(gZ=gZ, d=d, bank=dict(nelem=nelem, Z=Z, frac=F, energy=energy), cand=rng.permutation(nc).astype(np.int32), query_c=qc, query_e=qe)


def one_group(case, cand=None, q_rows=None):
    """The CSR arrays of one group over a case's queries."""
    cand = case["cand"] if cand is None else np.asarray(cand, np.int32)
    q_rows = np.arange(len(case["query_e"]), dtype=np.int32) if q_rows is None else np.asarray(q_rows, np.int32)
    gZ = np.zeros((1, MAX_ELEMS), np.int32)
    gZ[0, :case["d"]] = case["gZ"]
    return dict(grp_nelem=np.array([case["d"]], np.int32), grp_Z=gZ, grp_q_off=np.array([0, len(q_rows)], np.int32), q_idx=q_rows,
                grp_c_off=np.array([0, len(cand)], np.int32), c_idx=cand)


def merge_cases(cases):
    """Several cases as ONE call: the banks stacked, one group per case over its own rows, the queries stacked.  Returns (bank, groups,
    query_c, query_e)."""
    bank = {k: np.concatenate([c["bank"][k] for c in cases]) for k in ("nelem", "Z", "frac", "energy")}
    G = len(cases)
    gZ, q_off, c_off, q_idx, c_idx, row0, q0 = np.zeros((G, MAX_ELEMS), np.int32), [0], [0], [], [], 0, 0
    for g, c in enumerate(cases):
        gZ[g, :c["d"]] = c["gZ"]
        q_idx += list(range(q0, q0 + len(c["query_e"])))
        c_idx += [int(r) + row0 for r in c["cand"]]
        q_off.append(len(q_idx))
        c_off.append(len(c_idx))
        row0 += len(c["bank"]["nelem"])
        q0 += len(c["query_e"])
    i32 = lambda x: np.asarray(x, np.int32).reshape(-1)
    groups = dict(grp_nelem=i32([c["d"] for c in cases]), grp_Z=gZ, grp_q_off=i32(q_off), q_idx=i32(q_idx), grp_c_off=i32(c_off), c_idx=i32(c_idx))
    return bank, groups, np.concatenate([c["query_c"] for c in cases]), np.concatenate([c["query_e"] for c in cases])
