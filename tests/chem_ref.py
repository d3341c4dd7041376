"""The restatement of the composition-validity rule (include/matinvent_hip_chem.h) in plain Python integers: the enumeration is
`itertools.product` over the oxidation-state lists, the Pauling test is the literal loop over pairs.  A numpy mixed-radix form serves the
large N; the two are asserted equal on every small case by tests/test_chem_host.py.  Nothing here reads matinvent_amd's arithmetic: the
table is the JSON-shaped dict, the ranks are formed here from the floats."""
import itertools
import math
from functools import reduce

import numpy as np

SYMBOLS = ("X H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y Zr Nb Mo Tc "
           "Ru Rh Pd Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir Pt Au Hg Tl Pb Bi "
           "Po At Rn Fr Ra Ac Th Pa U Np Pu Am Cm Bk Cf Es Fm Md No Lr Rf Db Sg Bh Hs Mt Ds Rg Cn Nh Fl Mc Lv Ts Og").split()
Z_OF = {s: z for z, s in enumerate(SYMBOLS) if z}
MAX_ELEMS, MAX_STATES, CHUNK = 8, 32, 65536
STATUS = ("ENUMERATED", "ELEMENTAL", "ALLOY", "BAD_INPUT", "TOO_MANY_ELEMENTS", "UNKNOWN_ELEMENT", "NO_STATES", "TOO_MANY_COMBOS")
CODE = {s: i for i, s in enumerate(STATUS)}
SMALL = 200_000   # below this N the itertools form runs (and, in the CPU tests, the numpy form beside it)


def by_z(table):
    """{Z: (ox list, eneg or None, metal)} and {Z: rank} of a JSON-shaped table {"Na": {"ox": [...], "eneg": 0.93, "metal": True}}."""
    rows = {Z_OF[s]: (list(r.get("ox") or []), r.get("eneg"), bool(r.get("metal"))) for s, r in table.items()}
    levels = sorted(set(float(r[1]) for r in rows.values() if r[1] is not None))
    rank = {z: (levels.index(float(r[1])) if r[1] is not None else -1) for z, r in rows.items()}
    return rows, rank


def passes(states, ranks):
    """The literal Pauling test of one neutral combination."""
    if any(r < 0 for r in ranks):
        return False
    for a in range(len(states)):
        for b in range(len(states)):
            if states[a] > 0 > states[b] and not ranks[a] < ranks[b]:
                return False
    return True


def enumerate_itertools(lists, counts, ranks, use_pauling_test):
    n_neutral = n_valid = 0
    first, first_ox = -1, None
    for i, combo in enumerate(itertools.product(*lists)):
        if sum(o * c for o, c in zip(combo, counts)) != 0:
            continue
        n_neutral += 1
        if not use_pauling_test or passes(combo, ranks):
            n_valid += 1
            if first < 0:
                first, first_ox = i, list(combo)
    return n_neutral, n_valid, first, first_ox


def enumerate_numpy(lists, counts, ranks, use_pauling_test, block=1 << 20):
    radix = [len(l) for l in lists]
    N = math.prod(radix)
    arrs = [np.asarray(l, dtype=np.int64) for l in lists]
    n_neutral = n_valid = 0
    first, first_ox = -1, None
    unranked = any(r < 0 for r in ranks)
    for lo in range(0, N, block):
        idx = np.arange(lo, min(N, lo + block), dtype=np.int64)
        rest, states = idx.copy(), [None] * len(lists)
        for e in range(len(lists) - 1, -1, -1):   # the last element is the fastest digit
            states[e] = arrs[e][rest % radix[e]]
            rest //= radix[e]
        total = sum(s * c for s, c in zip(states, counts))
        keep = np.nonzero(total == 0)[0]
        n_neutral += len(keep)
        if len(keep) == 0:
            continue
        st = [s[keep] for s in states]
        ok = np.ones(len(keep), dtype=bool)
        if use_pauling_test:
            if unranked:
                ok[:] = False
            for a in range(len(lists)):
                for b in range(len(lists)):
                    if not ranks[a] < ranks[b]:
                        ok &= ~((st[a] > 0) & (st[b] < 0))
        n_valid += int(ok.sum())
        if first < 0 and ok.any():
            k = int(np.nonzero(ok)[0][0])
            first, first_ox = int(idx[keep[k]]), [int(s[k]) for s in st]
    return n_neutral, n_valid, first, first_ox


def one(types, table, use_pauling_test=True, include_alloys=True, max_combos=10_000_000, method="auto"):
    """Every output of one crystal as a dict (atom_ox: a list per atom)."""
    types = [int(t) for t in types]
    out = dict(valid=False, status=CODE["BAD_INPUT"], n_elems=0, elems=[0] * 8, counts=[0] * 8, n_combos=0, n_neutral=0, n_valid=0, first=-1, first_ox=[0] * 8,
               atom_ox=[0] * len(types))
    if len(types) == 0 or any(not 1 <= t <= 118 for t in types):
        return out
    rows, rank = by_z(table)
    elems = sorted(set(types))
    cnt = [types.count(z) for z in elems]
    g = reduce(math.gcd, cnt)
    cnt = [c // g for c in cnt]
    E = len(elems)
    out["n_elems"] = E
    out["elems"] = (elems + [0] * 8)[:8]
    out["counts"] = (cnt + [0] * 8)[:8]

    def done(status, valid):
        out["status"], out["valid"] = CODE[status], valid
        return out

    if E == 1:
        return done("ELEMENTAL", True)
    if E > MAX_ELEMS:
        return done("TOO_MANY_ELEMENTS", False)
    if any(z not in rows for z in elems):
        return done("UNKNOWN_ELEMENT", False)
    if include_alloys and all(rows[z][2] for z in elems):
        return done("ALLOY", True)
    lists = [rows[z][0] for z in elems]
    N = math.prod(len(l) for l in lists)
    out["n_combos"] = N
    if any(len(l) == 0 for l in lists):
        return done("NO_STATES", False)
    if N > max_combos:
        return done("TOO_MANY_COMBOS", False)
    ranks = [rank[z] for z in elems]
    if method == "auto":
        method = "itertools" if N <= SMALL else "numpy"
    f = enumerate_itertools if method == "itertools" else enumerate_numpy
    n_neutral, n_valid, first, first_ox = f(lists, cnt, ranks, use_pauling_test)
    out["n_neutral"], out["n_valid"], out["first"] = n_neutral, n_valid, first
    if first >= 0:
        out["first_ox"] = (first_ox + [0] * 8)[:8]
        out["atom_ox"] = [first_ox[elems.index(t)] for t in types]
    return done("ENUMERATED", n_valid > 0)


_cache = {}


def batch(crystals, table, table_key=None, **kw):
    """The outputs of a list of crystals (lists of atomic numbers) as the arrays of chemistry.ValidityResult.  With `table_key`, a crystal's
    row is computed once per (table_key, sorted types, keywords) and shared: the rule is a function of the composition, and atom_ox is
    re-spread over the crystal's own atom order."""
    rows = []
    for types in crystals:
        types = [int(t) for t in types]
        if table_key is None:
            rows.append(one(types, table, **kw))
            continue
        key = (table_key, tuple(sorted(types)), tuple(sorted(kw.items())))
        if key not in _cache:
            _cache[key] = one(sorted(types), table, **kw)
        r = dict(_cache[key])
        if r["first"] >= 0:
            r["atom_ox"] = [r["first_ox"][r["elems"].index(t)] for t in types]
        else:
            r["atom_ox"] = [0] * len(types)
        rows.append(r)
    i32, i64 = np.int32, np.int64
    return dict(valid=np.array([r["valid"] for r in rows], dtype=bool), status=np.array([r["status"] for r in rows], i32),
                n_elems=np.array([r["n_elems"] for r in rows], i32), elems=np.array([r["elems"] for r in rows], i32).reshape(-1, 8),
                counts=np.array([r["counts"] for r in rows], i32).reshape(-1, 8), n_combos=np.array([r["n_combos"] for r in rows], i64),
                n_neutral=np.array([r["n_neutral"] for r in rows], i64), n_valid=np.array([r["n_valid"] for r in rows], i64),
                first=np.array([r["first"] for r in rows], i64), first_ox=np.array([r["first_ox"] for r in rows], i32).reshape(-1, 8),
                atom_ox=np.array([o for r in rows for o in r["atom_ox"]], i32))


KEYS = ("valid", "status", "n_elems", "elems", "counts", "n_combos", "n_neutral", "n_valid", "first", "first_ox", "atom_ox")
