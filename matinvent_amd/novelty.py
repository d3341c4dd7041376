"""Uniqueness and novelty on structure fingerprints: the U and N of the reference's SUN filter (pipeline/filters/opt_filter.py:OptFilter with
metrics [validity, novel, unique, stable]).

The relation is the one of the structure-resolved memories (memory.py): two crystals are the same structure when they share the
reduced formula and their fingerprints (`structure.fingerprints`) lie within `fp_tol` in d = (1 - u1 . u2) / 2; a flagged crystal (no
fingerprint: more than 8 species, a degenerate cell) matches by formula alone.  What is new is the part that scales: a device-resident
`FingerprintBank` of reference rows and one HIP call (`mi_fp_match`, include/matinvent_hip_match.h) that finds, for every record of a
batch, the nearest bank row of its formula and the number of rows within the tolerance.

  * `novel_mask`: no bank row of the record's formula within fp_tol.
  * `unique_mask`: leader clustering in list order within each formula -- record i is kept iff no earlier KEPT record of its formula lies
    within fp_tol -- the relation `ReplayBuffer.extend` and `LongTimeMem._find` use.  This is a stated choice: mattergen's own `is_unique`
    rule is [UPSTREAM-UNVERIFIED], and its matcher is pymatgen's StructureMatcher, which is not reproduced.
  * `UNFilter`: both behind the reference's filter call shape, for `sample_cfg.filter`.

"stable" is stability.SUNFilter's (the energy above the convex hull of a phase bank), which owns a UNFilter for U and N; this
class keeps refusing the name.  "synthesizable" stays out of scope."""
import ctypes as C

import numpy as np
import torch

from .memory import _fingerprints_of, _formula, _species
from .structure import FP_NBINS, FP_R_MAX, FP_SIGMA, FP_TOL

MAX_SPECIES, MAX_BLOCKS = 8, 36   # include/matinvent_hip_fp.h


def round4(n):
    return (int(n) + 3) // 4 * 4


def record_ncols(record, nbins):
    """The leading columns of a record's fingerprint row that can be non-zero: blocks(m) nbins for its m species (m <= 8)."""
    m = len(set(_species(record)))
    return (m * (m + 1) // 2) * int(nbins) if 1 <= m <= MAX_SPECIES else 0


class FingerprintBank:
    """An append-only bank of fingerprint rows on the device: one flat float32 buffer, row r at element offset start[r] with len[r] floats
    (its own ncols rounded up to a multiple of 4, zero padding, every start a multiple of 4), both arrays growing by doubling, and a host
    index reduced formula -> row numbers.  A record whose fingerprint is flagged (status != 0) is remembered by its formula alone and owns
    no row."""

    def __init__(self, nbins=FP_NBINS, r_max=FP_R_MAX, sigma=FP_SIGMA, fp_tol=FP_TOL, device="cuda"):
        self.nbins, self.r_max, self.sigma, self.fp_tol = int(nbins), float(r_max), float(sigma), float(fp_tol)
        self.device = torch.device(device)
        self.rows = torch.zeros(1024, dtype=torch.float32, device=self.device)
        self.start = torch.zeros(64, dtype=torch.int64, device=self.device)
        self.length = torch.zeros(64, dtype=torch.int32, device=self.device)
        self.host_start, self.host_len = np.zeros(0, np.int64), np.zeros(0, np.int32)   # host mirrors: what `match` validates against
        self.n_floats = 0
        self.index = {}          # reduced formula -> [row, ...]
        self.flagged = {}        # reduced formula -> count of flagged records
        self.row_formula = []

    @property
    def fp_args(self):
        return {"nbins": self.nbins, "r_max": self.r_max, "sigma": self.sigma}

    def __len__(self):
        return len(self.row_formula)

    @property
    def formulas(self):
        return sorted(set(self.index) | set(self.flagged))

    def has_formula(self, formula):
        return formula in self.index or formula in self.flagged

    @staticmethod
    def _grown(t, need):
        if need <= t.numel():
            return t
        cap = t.numel()
        while cap < need:
            cap *= 2
        out = torch.zeros(cap, dtype=t.dtype, device=t.device)
        out[: t.numel()] = t
        return out

    def add_rows(self, formulas, ncols, fp, status):
        """Append one row per entry with status 0 (fp[i, :ncols[i]], padded), remember the others by formula.  Returns the row numbers
        (-1 for a flagged entry)."""
        if not isinstance(fp, (list, tuple)):   # (a list: rows of their own lengths)
            fp = np.asarray(fp, np.float32).reshape(len(formulas), -1)
        out, chunks, starts, lens = [], [], [], []
        at = self.n_floats
        for i, f in enumerate(formulas):
            n = int(ncols[i])
            if int(status[i]) != 0 or n <= 0:
                self.flagged[f] = self.flagged.get(f, 0) + 1
                out.append(-1)
                continue
            if n > len(fp[i]):
                raise ValueError(f"FingerprintBank.add: record {i} needs {n} columns, its row has {len(fp[i])}")
            ln = round4(n)
            row = np.zeros(ln, np.float32)
            row[:n] = np.asarray(fp[i], np.float32)[:n]
            chunks.append(row)
            starts.append(at)
            lens.append(ln)
            at += ln
            out.append(len(self.row_formula))
            self.index.setdefault(f, []).append(len(self.row_formula))
            self.row_formula.append(f)
        if chunks:
            m0, m1 = len(self.host_start), len(self.host_start) + len(chunks)
            self.rows = self._grown(self.rows, at)
            self.start, self.length = self._grown(self.start, m1), self._grown(self.length, m1)
            self.rows[self.n_floats:at] = torch.from_numpy(np.concatenate(chunks)).to(self.device)
            self.start[m0:m1] = torch.tensor(starts, dtype=torch.int64).to(self.device)
            self.length[m0:m1] = torch.tensor(lens, dtype=torch.int32).to(self.device)
            self.host_start = np.concatenate([self.host_start, np.asarray(starts, np.int64)])
            self.host_len = np.concatenate([self.host_len, np.asarray(lens, np.int32)])
            self.n_floats = at
        return out

    def add(self, records, fingerprints=None):
        if len(records) == 0:
            return []
        fp, status = _fingerprints_of(records, fingerprints, self.fp_args)
        return self.add_rows([_formula(r) for r in records], [record_ncols(r, self.nbins) for r in records], fp, status)

    def host_rows(self):
        """The rows as a list of host arrays (one read-back)."""
        flat = self.rows[: self.n_floats].cpu().numpy()
        return [flat[s:s + n] for s, n in zip(self.host_start, self.host_len)]

    def save(self, path):
        fl = sorted(self.flagged)
        with open(path, "wb") as f:
            np.savez(f, rows=self.rows[: self.n_floats].cpu().numpy(), lengths=self.host_len, formulas=np.array(self.row_formula, dtype=str),
                     flagged_formulas=np.array(fl, dtype=str), flagged_counts=np.array([self.flagged[k] for k in fl], np.int64),
                     nbins=np.int64(self.nbins), r_max=np.float64(self.r_max), sigma=np.float64(self.sigma))
        return path

    @classmethod
    def load(cls, path, nbins=FP_NBINS, r_max=FP_R_MAX, sigma=FP_SIGMA, fp_tol=FP_TOL, device="cuda"):
        with np.load(path, allow_pickle=False) as z:
            have = (int(z["nbins"]), float(z["r_max"]), float(z["sigma"]))
            if have != (int(nbins), float(r_max), float(sigma)):
                raise ValueError(f"FingerprintBank.load: {path} holds fingerprints of (nbins, r_max, sigma) = {have}, "
                                 f"asked for {(int(nbins), float(r_max), float(sigma))}: rows of different parameters do not compare")
            rows, lengths, formulas = z["rows"].astype(np.float32), z["lengths"].astype(np.int64), [str(s) for s in z["formulas"]]
            flagged = {str(k): int(v) for k, v in zip(z["flagged_formulas"], z["flagged_counts"])}
        if len(lengths) != len(formulas) or int(lengths.sum()) != len(rows) or (lengths % 4).any() or (lengths <= 0).any():
            raise ValueError(f"FingerprintBank.load: {path} is inconsistent ({len(formulas)} formulas, {len(lengths)} lengths summing to "
                             f"{int(lengths.sum())}, {len(rows)} floats)")
        bank = cls(nbins, r_max, sigma, fp_tol, device)
        width = int(lengths.max()) if len(lengths) else 4
        fp, at = np.zeros((len(lengths), width), np.float32), 0
        for i, n in enumerate(lengths):
            fp[i, :n] = rows[at:at + n]
            at += int(n)
        bank.add_rows(formulas, lengths, fp, np.zeros(len(lengths), np.int64))
        bank.flagged = flagged
        return bank

    @classmethod
    def from_records(cls, records, fingerprints=None, **kw):
        bank = cls(**kw)
        bank.add(records, fingerprints)
        return bank


# ---- the groups ---------------------------------------------------------------------------------------------------------------------------
def build_groups(formulas, ncols, status, bank, candidates=None):
    """The CSR arrays of one call: a group per reduced formula among the records with status 0, in order of first appearance; its queries
    in list order; its candidates the bank's rows of that formula (or `candidates[formula]`).  A formula absent from the bank is a group
    without candidates; flagged records are in no group."""
    order, members = [], {}
    for i, f in enumerate(formulas):
        if int(status[i]) != 0 or int(ncols[i]) <= 0:
            continue
        if f not in members:
            members[f] = []
            order.append(f)
        members[f].append(i)
    q_off, c_off, q_idx, c_idx, g_ncols = [0], [0], [], [], []
    for f in order:
        q_idx += members[f]
        c_idx += list((candidates if candidates is not None else bank.index).get(f, []))
        q_off.append(len(q_idx))
        c_off.append(len(c_idx))
        g_ncols.append(int(ncols[members[f][0]]))
    i32 = lambda x: np.asarray(x, np.int32).reshape(-1)
    return dict(formulas=order, grp_q_off=i32(q_off), q_idx=i32(q_idx), grp_c_off=i32(c_off), c_idx=i32(c_idx), grp_ncols=i32(g_ncols))


def validate_groups(groups, Q, row_stride, bank_len, ncols=None):
    """Everything the kernel's guard would skip is refused here, before any upload: offsets that are not ascending CSR offsets, an index
    out of range, a query in two groups, a candidate whose stored length differs from the group's rounded ncols, a row_stride that is no
    multiple of 4 or shorter than a group's length."""
    q_off, c_off, q_idx, c_idx, g_ncols = (np.asarray(groups[k], np.int64) for k in ("grp_q_off", "grp_c_off", "q_idx", "c_idx", "grp_ncols"))
    G = len(g_ncols)
    if len(q_off) != G + 1 or len(c_off) != G + 1:
        raise ValueError(f"fp match: {G} groups need {G + 1} offsets, got {len(q_off)} and {len(c_off)}")
    for name, off, n in (("grp_q_off", q_off, len(q_idx)), ("grp_c_off", c_off, len(c_idx))):
        if off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
            raise ValueError(f"fp match: {name} is not an ascending offset array from 0 to {n}")
    if row_stride % 4 or row_stride <= 0:
        raise ValueError(f"fp match: row_stride = {row_stride} is not a positive multiple of 4")
    if len(q_idx) and (q_idx.min() < 0 or q_idx.max() >= Q):
        raise ValueError(f"fp match: a query index outside 0..{Q - 1}")
    if len(np.unique(q_idx)) != len(q_idx):
        raise ValueError("fp match: a query row appears in more than one place")
    M = len(bank_len)
    if len(c_idx) and (c_idx.min() < 0 or c_idx.max() >= M):
        raise ValueError(f"fp match: a candidate index outside 0..{M - 1}")
    for g in range(G):
        n = int(g_ncols[g])
        if not 1 <= n <= row_stride or n > MAX_BLOCKS * 64:
            raise ValueError(f"fp match: group {g} has ncols = {n}, rows have {row_stride} columns")
        if ncols is not None and any(int(ncols[q]) != n for q in q_idx[q_off[g]:q_off[g + 1]]):
            raise ValueError(f"fp match: group {g} mixes row lengths")
        lens = np.asarray(bank_len, np.int64)[c_idx[c_off[g]:c_off[g + 1]]]
        if (lens != round4(n)).any():
            raise ValueError(f"fp match: group {g} (ncols {n}) lists a bank row of length {int(lens[lens != round4(n)][0])}, not {round4(n)}")
    return True


# ---- the kernel call ----------------------------------------------------------------------------------------------------------------------
class _Call:
    """One prepared mi_fp_match call: the argument block and the device arrays it points into (`launch` enqueues, `read` copies back)."""

    def __init__(self, args, keep, out, Q, G, nq_g, nc_g, pair_off, pairs):
        self.args, self.keep, self.out, self.Q, self.G, self.nq_g, self.nc_g, self.pair_off, self.pairs = args, keep, out, Q, G, nq_g, nc_g, pair_off, pairs

    def launch(self):
        from . import _lib
        _lib.check(_lib.load().mi_fp_match(C.byref(self.args), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "mi_fp_match")

    def read(self):
        Q, host, mats = self.Q, self.out.cpu().numpy(), None
        if self.pairs:
            flat = host[4 * Q:].view(np.float32)
            mats = [flat[self.pair_off[g]:self.pair_off[g + 1]].reshape(int(self.nq_g[g]), int(self.nc_g[g])) for g in range(self.G)]
        return (host[:Q].view(np.float32).copy(), host[Q:2 * Q].astype(np.int64), host[2 * Q:3 * Q].astype(np.int64),
                host[3 * Q:4 * Q].astype(np.int64), mats)


def _run_kernel(query, groups, bank, tol, pairs=False, chunk=0):
    """One mi_fp_match call: `query` [Q][row_stride] (numpy float32 or a device tensor), the validated `groups`, `bank`.  One upload of
    the integer arrays, one enqueue, one read-back.  Returns (best_dist [Q] float32, best_idx [Q], n_within [Q], status [Q], pair matrices
    per group or None)."""
    call = prepare_call(query, groups, bank, tol, pairs, chunk)
    if call is None:
        Q = len(query)
        return (np.full(Q, np.inf, np.float32), np.full(Q, -1, np.int64), np.zeros(Q, np.int64), np.zeros(Q, np.int64), [] if pairs else None)
    call.launch()
    return call.read()


def prepare_call(query, groups, bank, tol, pairs=False, chunk=0):
    """The plan, the upload and the argument block of one call (None when there is nothing to do)."""
    from . import _lib
    lib = _lib.load()
    dev = bank.device
    if dev.type != "cuda":
        raise RuntimeError("fp match runs on the GPU: the bank lives on " + str(dev))
    q = (query if torch.is_tensor(query) else torch.from_numpy(np.ascontiguousarray(query, np.float32))).to(dev).float().contiguous()
    Q, stride = int(q.shape[0]), int(q.shape[1])
    G = len(groups["grp_ncols"])
    nq_g, nc_g = np.diff(groups["grp_q_off"]).astype(np.int64), np.diff(groups["grp_c_off"]).astype(np.int64)
    if G == 0 or Q == 0:
        return None
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int))
    q_off, c_off = np.ascontiguousarray(groups["grp_q_off"], np.int32), np.ascontiguousarray(groups["grp_c_off"], np.int32)
    n_items, n_parts = C.c_int64(), C.c_int64()
    used = lib.mi_fp_match_plan(ip(q_off), ip(c_off), G, int(chunk), None, None, C.byref(n_items), C.byref(n_parts))
    _lib.check(0 if used > 0 else used, "mi_fp_match_plan")
    items = np.zeros(max(1, n_items.value) * _lib.FP_MATCH_ITEM_INTS, np.int32)
    part_off = np.zeros(G + 1, np.int32)
    used = lib.mi_fp_match_plan(ip(q_off), ip(c_off), G, int(used), ip(items), ip(part_off), C.byref(n_items), C.byref(n_parts))
    _lib.check(0 if used > 0 else used, "mi_fp_match_plan")
    parts = [q_off, np.ascontiguousarray(groups["q_idx"], np.int32), c_off, np.ascontiguousarray(groups["c_idx"], np.int32),
             np.ascontiguousarray(groups["grp_ncols"], np.int32), items, part_off]
    parts = [p if len(p) else np.zeros(1, np.int32) for p in parts]
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    ints = torch.from_numpy(np.concatenate(parts)).to(dev)
    pair_off = np.concatenate([[0], np.cumsum(nq_g * nc_g)]).astype(np.int64)
    pair_floats = int(pair_off[-1]) if pairs else 0
    out = torch.zeros(4 * Q + pair_floats, dtype=torch.int32, device=dev)
    out[:Q] = 0x7F800000          # +inf as fp32 bits: the rows of queries that belong to no group
    out[Q:2 * Q] = -1
    if pair_floats:
        out[4 * Q:] = 0x7FC00000   # nan: a pair the guard skipped stays visible
    pair_off_dev = torch.from_numpy(pair_off[:-1].copy()).to(dev) if pairs else None
    work = torch.empty(int(lib.mi_fp_match_workspace(n_parts.value)) // 4, dtype=torch.int32, device=dev)
    at = lambda t, k=0: C.c_void_p(t.data_ptr() + 4 * int(k))
    a = _lib.FpMatchArgs()
    a.query, a.bank, a.bank_start, a.bank_len = at(q), at(bank.rows), at(bank.start), at(bank.length)
    a.grp_q_off, a.q_idx, a.grp_c_off, a.c_idx, a.grp_ncols, a.items, a.grp_part_off = (at(ints, offs[k]) for k in range(7))
    a.workspace = at(work)
    a.best_dist, a.best_idx, a.n_within, a.status = at(out), at(out, Q), at(out, 2 * Q), at(out, 3 * Q)
    a.pair_dist = at(out, 4 * Q) if pairs else None
    a.pair_off = at(pair_off_dev) if pairs else None
    a.bank_floats, a.pair_floats = int(bank.n_floats), pair_floats
    a.Q, a.row_stride, a.M, a.G = Q, stride, len(bank), G
    a.nnz_q, a.nnz_c, a.n_items, a.n_partials = len(groups["q_idx"]), len(groups["c_idx"]), int(n_items.value), int(n_parts.value)
    a.max_ncols, a.tol = int(max(groups["grp_ncols"])), float(tol)
    return _Call(a, (q, ints, pair_off_dev, work, bank.rows, bank.start, bank.length), out, Q, G, nq_g, nc_g, pair_off, pairs)


def _match(formulas, ncols, fp, status, bank, tol, pairs=False, candidates=None):
    groups = build_groups(formulas, ncols, status, bank, candidates)
    fp = fp if torch.is_tensor(fp) else np.asarray(fp, np.float32).reshape(len(formulas), -1)
    stride = int(fp.shape[1]) if len(formulas) else 4
    validate_groups(groups, len(formulas), stride, bank.host_len, ncols)
    if len(formulas) == 0 or len(groups["grp_ncols"]) == 0:
        Q = len(formulas)
        return groups, (np.full(Q, np.inf, np.float32), np.full(Q, -1, np.int64), np.zeros(Q, np.int64), np.zeros(Q, np.int64), [] if pairs else None)
    res = _run_kernel(fp, groups, bank, tol, pairs)
    if res[3].any():
        raise RuntimeError("fp match: the kernel's guard skipped a candidate that the host validation had passed")
    return groups, res


def match(records, bank, fingerprints=None, pairs=False):
    """Per record (best_dist, best_idx, n_within) against the bank's rows of its reduced formula, within bank.fp_tol: three arrays (and,
    with pairs=True, a dict formula -> [queries of the formula][bank rows of the formula] of distances).  (inf, -1, 0) for a record whose
    formula the bank does not hold, and for a flagged record."""
    fp, status = _fingerprints_of(records, fingerprints, bank.fp_args)
    formulas, ncols = [_formula(r) for r in records], [record_ncols(r, bank.nbins) for r in records]
    groups, (bd, bi, nw, _, mats) = _match(formulas, ncols, fp, status, bank, bank.fp_tol, pairs)
    if pairs:
        return bd, bi, nw, dict(zip(groups["formulas"], mats))
    return bd, bi, nw


def novel_mask(records, bank, fingerprints=None):
    """True where no bank row of the record's reduced formula lies within bank.fp_tol.  A formula absent from the bank is novel; a flagged
    record matches by formula alone (the memories' convention): novel only if the bank has nothing of its formula."""
    if len(records) == 0:
        return np.zeros(0, bool)
    fp, status = _fingerprints_of(records, fingerprints, bank.fp_args)
    formulas, ncols = [_formula(r) for r in records], [record_ncols(r, bank.nbins) for r in records]
    _, (_, _, nw, _, _) = _match(formulas, ncols, fp, status, bank, bank.fp_tol)
    flagged = np.array([int(s) != 0 or n <= 0 for s, n in zip(status, ncols)])
    return np.where(flagged, [not bank.has_formula(f) for f in formulas], nw == 0)


def resolve_leaders(d, tol):
    """Leader clustering in list order from a pair matrix d [n][n]: i is kept iff no earlier kept j has d[i][j] <= tol."""
    d = np.asarray(d)
    n = len(d)
    kept, blocked = [], np.zeros(n, bool)
    for i in range(n):
        if blocked[i]:
            continue
        kept.append(i)
        blocked[i + 1:] |= d[i + 1:, i] <= tol
    return kept


def unique_mask(records, fingerprints=None, fp_tol=FP_TOL, fp_args=None, device="cuda"):
    """Leader clustering in list order within each reduced formula: record i is kept iff no earlier KEPT record of its formula lies within
    fp_tol -- the relation ReplayBuffer.extend and LongTimeMem._find use; flagged records match by formula alone, among the flagged.  The
    batch is its own bank for this call: the kernel supplies every formula group's pair matrix, the host resolves the leaders from those
    floats.  A stated choice: mattergen's own `is_unique` rule is [UPSTREAM-UNVERIFIED] and its matcher is pymatgen's."""
    n = len(records)
    if n == 0:
        return np.zeros(0, bool)
    bank = FingerprintBank(fp_tol=fp_tol, device=device, **(fp_args or {}))
    fp, status = _fingerprints_of(records, fingerprints, bank.fp_args)
    formulas, ncols = [_formula(r) for r in records], [record_ncols(r, bank.nbins) for r in records]
    rows = bank.add_rows(formulas, ncols, fp, status)
    groups, (_, _, _, _, mats) = _match(formulas, ncols, fp, status, bank, bank.fp_tol, pairs=True)
    mask, seen_flagged = np.zeros(n, bool), set()
    for i, r in enumerate(rows):
        if r < 0 and formulas[i] not in seen_flagged:
            seen_flagged.add(formulas[i])
            mask[i] = True
    for g, d in enumerate(mats):
        members = groups["q_idx"][groups["grp_q_off"][g]:groups["grp_q_off"][g + 1]]
        for k in resolve_leaders(d, bank.fp_tol):
            mask[members[k]] = True
    return mask


def validity_first(smact, flt, data_list, structures, energies=None):
    """The metric "validity" of UNFilter / SUNFilter: `smact`'s mask over the records, `flt` over the valid ones, `valid_frac` in the metrics."""
    records = structures if structures is not None else data_list
    n = len(records)
    keep = np.asarray(smact(records), dtype=bool) if n else np.zeros(0, bool)
    pick = lambda xs: [x for x, k in zip(xs, keep) if k] if xs is not None else None
    data, strucs, metrics = flt(pick(data_list), pick(structures), None if energies is None else np.asarray(energies)[keep])
    return data, strucs, dict(metrics, valid_frac=float(keep.mean()) if n else 0.0)


class UNFilter:
    """The reference's filter call shape, `flt(data_list, structures, energies=None) -> (data, structures, metrics)`, for
    sample_cfg.filter: keeps the crystals that are unique within the batch and novel against the bank.  `reference_path`: a .npz bank
    (scripts/build_fingerprint_bank.py).  remember=True adds every crystal the filter passes to the bank, so that "novel" also means not
    yet scored in this run, across loops.  metrics: a subset of {"unique", "novel"}; "validity" is accepted and ignored (invalid_filter has
    run already) -- unless `smact` is given (a chemistry.SmactValidity, a path or its config mapping): then the composition test
    runs first, on the (relaxed) structures as the reference's second test does (opt_filter.py:179-180), only the valid ones go on to the
    other metrics -- whose fractions are then taken over the valid ones -- and `valid_frac` is reported.  One fingerprint call serves both masks."""

    NEEDS = {"stable": "a MatterSim relaxation and a convex-hull reference set downloaded from a hub",
             "synthesizable": "a synthesizability model and its downloaded weights"}

    def __init__(self, metrics=("unique", "novel"), reference_path=None, remember=False, fp_tol=FP_TOL, fp_args=None, device="cuda",
                 matcher="fingerprint", ltol=0.2, stol=0.3, angle_tol=5.0, primitive=False, symprec=0.1, smact=None, **ignored):
        if smact is not None:
            from .chemistry import make_smact
            smact = make_smact(smact)
        self.smact = smact
        if matcher not in ("fingerprint", "structure"):
            raise ValueError(f"UNFilter: matcher {matcher!r} is neither 'fingerprint' nor 'structure'")
        self.matcher, self.ltol, self.stol, self.angle_tol = matcher, float(ltol), float(stol), float(angle_tol)
        self.primitive, self.symprec = bool(primitive), float(symprec)   # the structure matcher on primitive cells
        metrics = [str(m) for m in metrics]
        for m in metrics:
            if m in self.NEEDS:
                raise ValueError(f"UNFilter: metric {m!r} is not built -- it needs {self.NEEDS[m]} (out of scope: no outside assets)")
            if m not in ("unique", "novel", "validity"):
                raise ValueError(f"UNFilter: metric {m!r} is none of 'unique', 'novel', 'validity'")
        self.metrics = tuple(m for m in ("unique", "novel") if m in metrics)
        self.validity = "validity" in metrics and self.smact is not None
        self.remember, self.fp_tol, self.fp_args, self.device = bool(remember), float(fp_tol), dict(fp_args or {}), device
        self.reference_path, self._bank = reference_path, None

    @property
    def bank(self):
        if self._bank is None and self.matcher == "structure":   # a StructureBank (.npz of scripts/build_structure_bank.py)
            from .matching import StructureBank
            self._bank = (StructureBank.load(self.reference_path, self.device, self.primitive, self.symprec) if self.reference_path else
                          StructureBank(self.device, self.primitive, self.symprec))
        if self._bank is None:   # on first use: constructing the filter touches no device
            kw = dict(fp_tol=self.fp_tol, device=self.device, **self.fp_args)
            self._bank = FingerprintBank.load(self.reference_path, **kw) if self.reference_path else FingerprintBank(**kw)
        return self._bank

    def structure_masks(self, records):
        """(unique, novel, match_rms_mean) under the structure matcher (matching.unique_mask / novel_mask): the mean is taken
        over the records that match a bank row, NaN when none does."""
        from . import matching
        uniq = matching.unique_mask(records, self.ltol, self.stol, self.angle_tol, self.device, self.primitive, self.symprec)
        novel, rms = matching.novel_mask(records, self.bank, self.ltol, self.stol, self.angle_tol, return_rms=True)
        hit = rms <= self.stol
        return uniq, novel, float(rms[hit].mean()) if hit.any() else float("nan")

    def __call__(self, data_list, structures, energies=None):
        if not self.validity:
            return self._filter(data_list, structures, energies)
        return validity_first(self.smact, self._filter, data_list, structures, energies)

    def _filter(self, data_list, structures, energies=None):
        records = structures if structures is not None else data_list
        n = len(records)
        bank = self.bank
        if n == 0:
            m = {"unique_frac": 0.0, "novel_frac": 0.0, "un_frac": 0.0, "bank_size": float(len(bank))}
            if self.matcher == "structure":
                m["match_rms_mean"] = float("nan")
            return data_list, structures, m
        if self.matcher == "structure":
            uniq, novel, rms_mean = self.structure_masks(records)
            keep = np.ones(n, bool)
            if "unique" in self.metrics:
                keep &= uniq
            if "novel" in self.metrics:
                keep &= novel
            idx = [i for i in range(n) if keep[i]]
            if self.remember and idx:
                bank.add([records[i] for i in idx])
            metrics = {"unique_frac": float(uniq.mean()), "novel_frac": float(novel.mean()), "un_frac": float((uniq & novel).mean()),
                       "bank_size": float(len(bank)), "match_rms_mean": rms_mean}
            pick = lambda xs: [xs[i] for i in idx] if xs is not None else None
            return pick(data_list), pick(structures), metrics
        fingerprints = _fingerprints_of(records, None, bank.fp_args)
        uniq = unique_mask(records, fingerprints, self.fp_tol, bank.fp_args, self.device)
        novel = novel_mask(records, bank, fingerprints)
        keep = np.ones(n, bool)
        if "unique" in self.metrics:
            keep &= uniq
        if "novel" in self.metrics:
            keep &= novel
        idx = [i for i in range(n) if keep[i]]
        if self.remember and idx:
            bank.add([records[i] for i in idx], (fingerprints[0][idx], fingerprints[1][idx]))
        metrics = {"unique_frac": float(uniq.mean()), "novel_frac": float(novel.mean()), "un_frac": float((uniq & novel).mean()),
                   "bank_size": float(len(bank))}
        pick = lambda xs: [xs[i] for i in idx] if xs is not None else None
        return pick(data_list), pick(structures), metrics
