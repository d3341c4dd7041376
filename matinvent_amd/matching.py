"""The structure matcher on the device (include/matinvent_hip_smatch.h): is it the same structure, how far apart, and which
atom is which.  Follows the algorithm of pymatgen's StructureMatcher step by step -- lattice maps within (ltol, angle_tol), candidate
translations from the rarest species, a species-constrained optimal assignment, an RMS displacement normalised by (V / n)^(1/3) compared
with stol -- and is not bit-compatible with it; the defaults ltol 0.2, stol 0.3, angle_tol 5 degrees are [UPSTREAM-UNVERIFIED].  With
primitive=True every crystal is reduced to its primitive cell first (symmetry.py, DESIGN 50: prepare -> mi_sym_find -> mi_sym_primitive
-> prepare), so two cells of one structure with different atom counts are compared; the default False compares cells as given.  Not
built: supercell search inside the matcher, the disordered matcher's substitutions, the second acceptance criterion on max_dist."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .structure import record_arrays

LTOL, STOL, ANGLE_TOL = 0.2, 0.3, 5.0   # pymatgen's defaults [UPSTREAM-UNVERIFIED]


class Prepared:
    """A prepared set on the device: the arrays of mi_sm_prepare (lat, inv [B, 9] float64; frac [N, 3] float64; types, perm [N]; spec_Z
    [B, 16]; spec_off [B, 17]; info [B, 4] = atoms, species, rarest species, status)."""

    def __init__(self, offsets, N, device, fill=None):
        B = len(offsets) - 1
        self.B, self.N, self.offsets = B, int(N), offsets
        z = (lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)) if fill is None else fill
        self.lat, self.inv, self.frac = z((B, 9), torch.float64), z((B, 9), torch.float64), z((max(N, 1), 3), torch.float64)
        self.types, self.perm = z((max(N, 1),), torch.int32), z((max(N, 1),), torch.int32)
        self.spec_Z, self.spec_off, self.info = z((B, 16), torch.int32), z((B, 17), torch.int32), z((B, 4), torch.int32)

    def struct(self):
        p = lambda t: t.data_ptr()
        return _lib.SmPrepared(p(self.offsets), p(self.lat), p(self.inv), p(self.frac), p(self.types), p(self.perm), p(self.spec_Z), p(self.spec_off),
                               p(self.info), self.B, self.N)

    @property
    def status(self):
        return self.info[:, 3]


def prepare_arrays(offsets, types, frac, lat, fill=None):
    """mi_sm_prepare on device tensors: offsets int32 [B + 1], types int32 [N], frac float32 [N, 3], lat float32 [B, 9 or 3 x 3].  `fill`
    builds the output tensors (tests poison them)."""
    lib = _lib.load()
    offsets, types = offsets.to(torch.int32).contiguous(), types.to(torch.int32).contiguous()
    frac, lat = frac.to(torch.float32).contiguous(), lat.to(torch.float32).contiguous()
    out = Prepared(offsets, types.numel(), offsets.device, fill)
    if out.B:
        st = out.struct()
        _lib.check(lib.mi_sm_prepare(types.data_ptr(), frac.data_ptr(), lat.data_ptr(), C.byref(st), torch.cuda.current_stream().cuda_stream), "mi_sm_prepare")
    return out


def prepare_primitive_arrays(offsets, types, frac, lat, tol):
    """The prepared set of the primitive cells: prepare -> mi_sym_find -> mi_sym_primitive -> prepare, nothing read back.
    tol: symmetry.tolerances of the crystals."""
    from . import symmetry
    prim, _ = symmetry.reduce_arrays(offsets, types, frac, lat, tol)
    return prepare_arrays(prim.offsets, prim.types, prim.frac, prim.lat)


def prepare(records, device="cuda", primitive=False, symprec=0.1):
    """A prepared set from host records (SimpleStructure / CrystalData-like): one upload, one launch.  primitive: of their primitive
    cells (symprec in A, symmetry.py's)."""
    na, types, frac, lat = record_arrays(records)
    offsets = torch.cat([torch.zeros(1, dtype=torch.long), na.cumsum(0)]).to(torch.int32)
    dev = torch.device(device)
    if primitive and len(records):
        from . import symmetry
        return prepare_primitive_arrays(offsets.to(dev), types.to(dev), frac.to(dev), lat.reshape(-1, 9).to(dev),
                                        symmetry.tolerances(na.numpy(), lat.numpy(), symprec))
    return prepare_arrays(offsets.to(dev), types.to(dev), frac.to(dev), lat.reshape(-1, 9).to(dev))


def _counts(prepared):
    """The atom counts of a prepared set on the host: one read."""
    return np.diff(prepared.offsets.cpu().numpy().astype(np.int64))


def match_pairs(set_a, set_b, pairs, ltol=LTOL, stol=STOL, angle_tol=ANGLE_TOL, permutation=False, maps=False, large_tile=False, fill=None):
    """mi_sm_match over (query row of set_a, candidate row of set_b) pairs [P, 2]: a dict of device tensors rms, max_dist [P] float64,
    best_map [P, 9], best_trans, n_maps, n_items, status [P], fit [P] (rms <= stol), and perm [P, 64] with permutation=True (query atom
    -> candidate atom in the callers' orders)."""
    lib = _lib.load()
    dev = set_a.lat.device
    pairs = torch.as_tensor(pairs, dtype=torch.int32, device=dev).reshape(-1, 2)
    P = len(pairs)
    pq, pc = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
    z = (lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)) if fill is None else fill
    out = {"rms": z((P,), torch.float64), "max_dist": z((P,), torch.float64), "best_map": z((P, 9), torch.int32), "best_trans": z((P,), torch.int32),
           "n_maps": z((P,), torch.int32), "n_items": z((P,), torch.int32), "status": z((P,), torch.int32)}
    if permutation:
        out["perm"] = z((P, _lib.SM_MAX_ATOMS), torch.int32)
    if maps:
        out["maps"] = z((P, _lib.SM_MAX_MAPS, 9), torch.int32)
    if P:
        p = lambda k: out[k].data_ptr() if k in out else None
        args = _lib.SmMatchArgs(set_a.struct(), set_b.struct(), pq.data_ptr(), pc.data_ptr(), p("rms"), p("max_dist"), p("best_map"), p("best_trans"),
                                p("n_maps"), p("n_items"), p("status"), p("perm"), p("maps"), float(ltol), math.cos(math.radians(float(angle_tol))), P,
                                1 if large_tile else 0)
        _lib.check(lib.mi_sm_match(C.byref(args), torch.cuda.current_stream().cuda_stream), "mi_sm_match")
    out["fit"] = out["rms"] <= float(stol)
    return out


def rms_dist(record_a, record_b, ltol=LTOL, stol=STOL, angle_tol=ANGLE_TOL, device="cuda", primitive=False, symprec=0.1):
    """(rms, max_dist) of the best map, translation and assignment, or None when the two are not comparable or have no lattice map."""
    s = prepare([record_a, record_b], device, primitive, symprec)
    r = match_pairs(s, s, [(0, 1)], ltol, stol, angle_tol)
    rms, md, st = float(r["rms"][0]), float(r["max_dist"][0]), int(r["status"][0])
    return (rms, md) if st == _lib.SM_OK and np.isfinite(rms) else None


def fit(record_a, record_b, ltol=LTOL, stol=STOL, angle_tol=ANGLE_TOL, device="cuda", primitive=False, symprec=0.1):
    """rms <= stol.  pymatgen's second criterion on max_dist is not reproduced."""
    d = rms_dist(record_a, record_b, ltol, stol, angle_tol, device, primitive, symprec)
    return d is not None and d[0] <= stol


def _key(record):
    from .memory import _formula, _species
    return _formula(record), len(_species(record))


class StructureBank:
    """An append-only reference set for the structure matcher.  The records' arrays (atom counts, atomic numbers, float32 coordinates and
    cells) are kept on the host, the prepared set on the device; it is prepared again, in one launch, at the first use after an append.
    A host index (reduced formula, atom count) -> rows selects a query's candidates.  save / load: an .npz of those arrays only.
    primitive=True: every record is reduced to its primitive cell as it is added (one read of the reduced arrays per append, none per
    match) and the index keys on the primitive atom count; queries are then reduced the same way."""

    def __init__(self, device="cuda", primitive=False, symprec=0.1):
        self.device, self.primitive, self.symprec = torch.device(device), bool(primitive), float(symprec)
        self.na, self.types, self.frac, self.lat, self.keys = [], [], [], [], []
        self.index, self.formulas, self._set = {}, set(), None

    def __len__(self):
        return len(self.keys)

    def add(self, records):
        if len(records) == 0:
            return
        na, types, frac, lat = record_arrays(records)
        keys = [_key(r) for r in records]
        if self.primitive:
            from . import symmetry
            off = torch.cat([torch.zeros(1, dtype=torch.long), na.cumsum(0)]).to(torch.int32)
            prim, _ = symmetry.reduce_arrays(off.to(self.device), types.to(self.device), frac.to(self.device), lat.reshape(-1, 9).to(self.device),
                                             symmetry.tolerances(na.numpy(), lat.numpy(), self.symprec))
            poff = prim.offsets.cpu().numpy().astype(np.int64)
            n = int(poff[-1])
            na, types, frac, lat = torch.from_numpy(np.diff(poff)), prim.types[:n].cpu(), prim.frac[:n].cpu(), prim.lat.cpu()
            keys = [(k[0], int(c)) for k, c in zip(keys, na.tolist())]
        self._add_arrays(na.numpy(), types.numpy(), frac.numpy(), lat.reshape(-1, 9).numpy(), keys)

    def _add_arrays(self, na, types, frac, lat, keys):
        for k in keys:
            self.index.setdefault(tuple(k), []).append(len(self.keys))
            self.formulas.add(k[0])
            self.keys.append(tuple(k))
        self.na.append(np.asarray(na, np.int64)), self.types.append(np.asarray(types, np.int32))
        self.frac.append(np.asarray(frac, np.float32).reshape(-1, 3)), self.lat.append(np.asarray(lat, np.float32).reshape(-1, 9))
        self._set = None

    def arrays(self):
        cat = lambda xs, empty: np.concatenate(xs) if xs else empty
        return (cat(self.na, np.zeros(0, np.int64)), cat(self.types, np.zeros(0, np.int32)), cat(self.frac, np.zeros((0, 3), np.float32)),
                cat(self.lat, np.zeros((0, 9), np.float32)))

    @property
    def prepared(self):
        if self._set is None:
            na, types, frac, lat = self.arrays()
            off = np.concatenate([[0], np.cumsum(na)]).astype(np.int32)
            t = lambda a: torch.from_numpy(a).to(self.device)
            self._set = prepare_arrays(t(off), t(types), t(frac), t(lat))
        return self._set

    def rows(self, key):
        return self.index.get(tuple(key), [])

    def save(self, path):
        na, types, frac, lat = self.arrays()
        np.savez(path, num_atoms=na, atom_types=types, frac_coords=frac, lattices=lat, formulas=np.array([k[0] for k in self.keys], dtype=str))
        return path

    @classmethod
    def load(cls, path, device="cuda", primitive=False, symprec=0.1):
        """primitive: the file's cells are taken as primitive already (a bank that was saved from a primitive=True bank)."""
        bank = cls(device, primitive, symprec)
        with np.load(path, allow_pickle=False) as z:
            na = z["num_atoms"]
            if len(na):
                bank._add_arrays(na, z["atom_types"], z["frac_coords"], z["lattices"], [(str(f), int(n)) for f, n in zip(z["formulas"], na)])
        return bank

    @classmethod
    def from_records(cls, records, device="cuda", primitive=False, symprec=0.1):
        bank = cls(device, primitive, symprec)
        bank.add(records)
        return bank


def novel_mask(records, bank, ltol=LTOL, stol=STOL, angle_tol=ANGLE_TOL, return_rms=False):
    """True where no bank row of the record's (reduced formula, atom count) fits it: one mi_sm_match call over every (record, row) pair.
    A record whose prepare status is not OK matches by formula alone (the memories' convention for flagged records): novel only if the
    bank holds nothing of its formula.  Never drops or reorders.  return_rms: also the smallest rms per record (inf without a fit)."""
    n = len(records)
    best = np.full(n, np.inf)
    if n == 0:
        return (np.zeros(0, bool), best) if return_rms else np.zeros(0, bool)
    keys = [_key(r) for r in records]
    q = prepare(records, bank.device, bank.primitive, bank.symprec)
    if bank.primitive:
        keys = [(k[0], int(c)) for k, c in zip(keys, _counts(q))]
    flagged = q.status.cpu().numpy() != _lib.SM_PREP_OK
    novel = np.ones(n, bool)
    pairs = [(i, row) for i in range(n) if not flagged[i] for row in bank.rows(keys[i])]
    if pairs:
        rms = match_pairs(q, bank.prepared, pairs, ltol, stol, angle_tol)["rms"].cpu().numpy()
        for (i, _), d in zip(pairs, rms):
            best[i] = min(best[i], d)
        novel = ~(best <= stol)
    for i in range(n):
        if flagged[i]:
            novel[i] = keys[i][0] not in bank.formulas
    return (novel, best) if return_rms else novel


def unique_mask(records, ltol=LTOL, stol=STOL, angle_tol=ANGLE_TOL, device="cuda", primitive=False, symprec=0.1):
    """Leader clustering in list order within each (reduced formula, atom count): record i is kept iff no earlier KEPT record fits it, the
    rule novelty.unique_mask documents; the pair matrix of every group comes from one mi_sm_match call and novelty.resolve_leaders reads
    it.  Records whose prepare status is not OK match by formula alone, among themselves: the first of a formula is kept.  primitive: the
    records are reduced to their primitive cells first and the groups key on the primitive atom count."""
    from .novelty import resolve_leaders
    n = len(records)
    mask = np.zeros(n, bool)
    if n == 0:
        return mask
    keys = [_key(r) for r in records]
    s = prepare(records, device, primitive, symprec)
    if primitive:   # the groups key on the primitive atom count
        keys = [(k[0], int(c)) for k, c in zip(keys, _counts(s))]
    flagged = s.status.cpu().numpy() != _lib.SM_PREP_OK
    groups, seen_flagged = {}, set()
    for i, k in enumerate(keys):
        if flagged[i]:
            if k[0] not in seen_flagged:
                seen_flagged.add(k[0])
                mask[i] = True
        else:
            groups.setdefault(k, []).append(i)
    pairs = [(g[a], g[b]) for g in groups.values() for a in range(len(g)) for b in range(a)]
    rms = match_pairs(s, s, pairs, ltol, stol, angle_tol)["rms"].cpu().numpy() if pairs else np.zeros(0)
    at = 0
    for g in groups.values():
        d = np.full((len(g), len(g)), np.inf)
        for a in range(len(g)):
            for b in range(a):
                d[a, b] = d[b, a] = rms[at]
                at += 1
        for k in resolve_leaders(d, stol):
            mask[g[k]] = True
    return mask
