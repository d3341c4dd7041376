"""Fingerprint matching (include/matinvent_hip_match.h) restated in numpy float64: the groups of a record list against a bank,
the pair distances d = (1 - u . v) / 2, the per-query reductions (nearest row with ties to the lowest bank index, count within the
tolerance), leader clustering from a 0/1 relation, the kernel's guard, and the error budget its documented summation order implies."""
import numpy as np

TILE = 8   # MI_FP_MATCH_TILE


def round4(n):
    return (int(n) + 3) // 4 * 4


def chain(ncols):
    """L(ncols) of the header: the longest chain of sequential additions of one pair's sum."""
    return 4 * ((round4(ncols) + 255) // 256) + 6


def budget(u, v, ncols):
    """|d_dev - d_64| <= (L + 8) 2^-24 1/2 sum |u_i v_i| + 2^-24: a floating-point sum of depth L (the products are exact inside the
    FMAs), plus one rounding each for the subtraction, the halving and the store."""
    u, v = np.asarray(u, np.float64)[:ncols], np.asarray(v, np.float64)[:ncols]
    return (chain(ncols) + 8) * 2.0 ** -24 * 0.5 * float(np.abs(u * v).sum()) + 2.0 ** -24


def distance(u, v):
    return 0.5 * (1.0 - float(np.dot(np.asarray(u, np.float64), np.asarray(v, np.float64))))


def pair_matrix(queries, bank_rows, ncols):
    """[nq][nc] float64 distances over the leading ncols columns."""
    q = np.asarray(queries, np.float64).reshape(len(queries), -1)[:, :ncols]
    c = np.asarray(bank_rows, np.float64).reshape(len(bank_rows), -1)[:, :ncols] if len(bank_rows) else np.zeros((0, ncols))
    return 0.5 * (1.0 - q @ c.T)


def reduce_pairs(d, cand_idx, tol):
    """Per query row of d [nq][nc]: (best_dist, best_idx, n_within); ties to the lowest bank index; (inf, -1, 0) without candidates."""
    cand_idx = np.asarray(cand_idx, np.int64)
    if len(cand_idx) == 0:
        return [(np.inf, -1, 0)] * len(d)
    out = []
    for row in np.asarray(d, np.float64).reshape(-1, len(cand_idx)):
        best = row.min()
        out.append((float(best), int(cand_idx[row == best].min()), int((row <= tol).sum())))
    return out


def match_groups(query, groups, bank_rows, bank_len, tol):
    """The whole call on the host.  groups: list of (q_rows, c_rows, ncols); bank_rows: list of 1-d arrays (each of its own padded
    length), bank_len their lengths.  Returns (best_dist [Q], best_idx [Q], n_within [Q], status [Q], pairs: list of [nq][nc] arrays with
    nan where the guard skipped the candidate).  Queries of no group keep (inf, -1, 0, 0)."""
    Q = len(query)
    best_d, best_i, within, status = np.full(Q, np.inf), np.full(Q, -1, np.int64), np.zeros(Q, np.int64), np.zeros(Q, np.int64)
    pairs = []
    for q_rows, c_rows, ncols in groups:
        ln = round4(ncols)
        good = [0 <= int(c) < len(bank_rows) and int(bank_len[int(c)]) == ln for c in c_rows]
        d = np.full((len(q_rows), len(c_rows)), np.nan)
        for k, c in enumerate(c_rows):
            if good[k]:
                d[:, k] = pair_matrix([query[q] for q in q_rows], [np.asarray(bank_rows[int(c)])[:ln]], ln)[:, 0] if len(q_rows) else 0
        pairs.append(d)
        keep = [k for k, g in enumerate(good) if g]
        red = reduce_pairs(d[:, keep], [int(c_rows[k]) for k in keep], tol)
        for j, q in enumerate(q_rows):
            best_d[q], best_i[q], within[q] = red[j]
            status[q] = 0 if all(good) else 1
    return best_d, best_i, within, status, pairs


def leaders_naive(same):
    """Leader clustering in list order: record i is kept iff no EARLIER KEPT record j has same[i][j].  The plain sequential loop."""
    same = np.asarray(same, bool)
    kept = []
    for i in range(len(same)):
        if not any(same[i][j] for j in kept):
            kept.append(i)
    return kept


def unique_mask(formulas, fp, status, tol):
    """Leader clustering within each formula on float64 distances; a flagged record (status != 0) matches by formula alone, among the
    flagged (the memories' convention)."""
    n = len(formulas)
    same = np.zeros((n, n), bool)
    for i in range(n):
        for j in range(n):
            if formulas[i] == formulas[j] and (status[i] == 0) == (status[j] == 0):
                same[i, j] = status[i] != 0 or distance(fp[i], fp[j]) <= tol
    mask = np.zeros(n, bool)
    mask[leaders_naive(same)] = True
    return mask


def novel_mask(formulas, fp, status, bank_formulas, bank_fp, bank_status, tol):
    """A record is novel iff no bank row of its formula lies within tol; a flagged record, iff the bank has nothing of its formula."""
    out = np.ones(len(formulas), bool)
    for i, f in enumerate(formulas):
        for j, g in enumerate(bank_formulas):
            if f != g:
                continue
            if status[i] != 0 or (bank_status[j] == 0 and distance(fp[i], bank_fp[j]) <= tol):
                out[i] = False
    return out


def unit_rows(n, ncols, width, seed):
    """n synthetic unit rows: drawn in float64, normalised, rounded to fp32, zero past ncols."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, ncols))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    out = np.zeros((n, width), np.float32)
    out[:, :ncols] = x.astype(np.float32)
    return out


# ---- the shared test case of the distance checks (CPU host program and GPU kernel) --------------------------------------------------------------
NCOLS = (1, 3, 5, 15, 64, 192, 2304)     # 5 and 15: nbins = 5, the zero-padded tail; 2304: the full width
NCAND = (0, 1, 3, 4, 5, 9, 257)          # around the query-tile height and the wave's four, and beyond one candidate chunk
NQUERY = (1, 2, 9)
WIDTH = 2304
TOL = 0.25


def distance_case(seed=7):
    """One call's worth: a group per (ncols, candidates, queries) of the three lists, every group with rows of its own.  Returns
    dict(query [Q][WIDTH] fp32, bank_rows: list of padded fp32 rows, bank_len, groups: list of (q_rows, c_rows, ncols)); the candidate lists
    are shuffled, the groups interleaved over the query matrix."""
    g = np.random.default_rng(seed)
    shapes = [(n, c, q) for n in NCOLS for c in NCAND for q in NQUERY]
    order = g.permutation(len(shapes))
    nq_total = sum(s[2] for s in shapes)
    q_slots = g.permutation(nq_total)
    query, bank_rows, groups, at = np.zeros((nq_total, WIDTH), np.float32), [], [], 0
    for k in order:
        ncols, nc, nq = shapes[k]
        rows = unit_rows(nq + nc, ncols, round4(ncols), seed * 1000 + int(k))
        q_rows = [int(x) for x in q_slots[at:at + nq]]
        at += nq
        for j, q in enumerate(q_rows):
            query[q, :round4(ncols)] = rows[j]
        first = len(bank_rows)
        bank_rows += [rows[nq + j] for j in range(nc)]
        groups.append((q_rows, [int(x) for x in first + g.permutation(nc)], ncols))
    return dict(query=query, bank_rows=bank_rows, bank_len=np.array([len(r) for r in bank_rows], np.int32), groups=groups)


def pack(groups, bank_rows):
    """The C entry's arrays from the lists: CSR int32 arrays, the flat bank with its starts and lengths."""
    i32 = lambda x: np.asarray(x, np.int32).reshape(-1)
    q_off, c_off, q_idx, c_idx, ncols = [0], [0], [], [], []
    for q_rows, c_rows, n in groups:
        q_idx += list(q_rows)
        c_idx += list(c_rows)
        q_off.append(len(q_idx))
        c_off.append(len(c_idx))
        ncols.append(n)
    lens = np.array([len(r) for r in bank_rows], np.int64)
    start = np.concatenate([[0], np.cumsum(lens)])[:-1].astype(np.int64) if len(lens) else np.zeros(0, np.int64)
    flat = np.concatenate(bank_rows).astype(np.float32) if len(bank_rows) else np.zeros(0, np.float32)
    return dict(grp_q_off=i32(q_off), q_idx=i32(q_idx), grp_c_off=i32(c_off), c_idx=i32(c_idx), grp_ncols=i32(ncols), bank=flat, bank_start=start,
                bank_len=lens.astype(np.int32))


def check_distances(case, best_d, best_i, within, status, pairs, tol, label=""):
    """The assertions of the distance test on one call's outputs (fp32 pair matrices per group): every pair within the documented budget of
    float64, best_dist bitwise the pair entry at best_idx, n_within the float64 count (no pair within 10 budgets of tol), empty groups
    (-1, 0, 0).  Prints the worst error / budget per ncols."""
    worst = {}
    for (q_rows, c_rows, ncols), d_dev in zip(case["groups"], pairs):
        ln = round4(ncols)
        assert d_dev.shape == (len(q_rows), len(c_rows)) and d_dev.dtype == np.float32
        for j, q in enumerate(q_rows):
            assert status[q] == 0
            if len(c_rows) == 0:
                assert best_i[q] == -1 and within[q] == 0 and np.isinf(best_d[q])
                continue
            u = case["query"][q, :ln]
            d64 = np.array([distance(u, case["bank_rows"][c]) for c in c_rows])
            bud = np.array([budget(u, case["bank_rows"][c], ln) for c in c_rows])
            err = np.abs(d_dev[j].astype(np.float64) - d64)
            worst[ncols] = max(worst.get(ncols, 0.0), float((err / bud).max()))
            assert (err <= bud).all(), (label, ncols, len(c_rows), float((err / bud).max()))
            assert (np.abs(d64 - tol) > 10 * bud).all(), "the test rows must keep every pair 10 budgets away from tol"
            assert within[q] == int((d64 <= tol).sum())
            k = c_rows.index(int(best_i[q]))
            assert np.float32(best_d[q]).tobytes() == d_dev[j, k].tobytes()
            assert d_dev[j, k] == d_dev[j].min() and best_i[q] == min(c for c, x in zip(c_rows, d_dev[j]) if x == d_dev[j].min())
    for ncols in sorted(worst):
        print(f"{label} ncols {ncols:5d}  L {chain(ncols):3d}  worst error / budget {worst[ncols]:.3f}")
    return worst
