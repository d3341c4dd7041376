"""Energy above the convex hull on the device: the S of the reference's SUN filter (pipeline/filters/opt_filter.py:OptFilter with metrics
[validity, novel, unique, stable]).

The reference takes this from pymatgen's PhaseDiagram inside mattergen's MetricsEvaluator: one Qhull build per chemical system, on the
host, per call.  Here the hull is never built.  A crystal's energy above the hull is the value of a small linear programme -- the cheapest
mixture of reference phases at the crystal's composition -- and `mi_hull_above` (include/matinvent_hip_hull.h) solves one per crystal, a
whole batch per call, against a `PhaseBank` that lives on the device.

  * `PhaseBank`: append-only rows (element list, atomic fractions, energy per atom); `candidates(element_set)` are the rows whose
    elements are a subset of the set.
  * `energy_above_hull(records, energies, bank)`: e_hull, e_above, the chemical potentials and the decomposition of every record.
  * `stable_mask(result, threshold)`: e_above <= threshold and the solver ended at an optimum.
  * `SUNFilter`: stable, unique and novel behind the reference's filter call shape, for `sample_cfg.filter`; U and N are a
    `novelty.UNFilter`'s.

The energies are whatever the caller relaxed with (`relax.Relaxer` returns the energies of a `PropertyPredictor`); the bank must hold
energies of the same model (scripts/build_phase_bank.py --predictor).  Out of scope: the MP2020 energy corrections, pymatgen's PhaseDiagram
object, "synthesizable", a bank on several GPUs, and any claim about the quality of stability labels -- no weight here is trained."""
import ctypes as C

import numpy as np
import torch

from .memory import _species

MAX_ELEMS = 8                 # include/matinvent_hip_hull.h
OK, NO_TERMINAL, UNBOUNDED, ITER_CAP, BAD_QUERY, NOT_RUN = 0, 1, 2, 3, 4, -1
FLAG_SKIPPED = 1
STABLE_THRESHOLD = 0.1        # eV/atom above the hull that still counts as stable: mattergen's default [UPSTREAM-UNVERIFIED]
OUTPUT_KEYS = ("e_hull", "e_above", "chempot", "decomp_idx", "decomp_frac", "iters", "status", "flags")


def composition(record):
    """(sorted atomic numbers, atomic fractions float64, atom count) of a record."""
    z = np.asarray(_species(record), np.int64)
    if len(z) == 0:
        return np.zeros(0, np.int64), np.zeros(0), 0
    el, cnt = np.unique(z, return_counts=True)
    return el, cnt / float(len(z)), len(z)


def element_mask(Z):
    """The 128-bit element mask of a list of atomic numbers as two uint64 words."""
    m = np.zeros(2, np.uint64)
    for z in Z:
        z = int(z)
        if not 0 < z < 128:
            raise ValueError(f"atomic number {z} outside 1..127")
        m[z // 64] |= np.uint64(1) << np.uint64(z % 64)
    return m


class PhaseBank:
    """An append-only bank of reference phases: per row the element count, the sorted atomic numbers [8], their atomic fractions [8]
    (float64) and the energy per atom (float64; NaN is kept and never priced).  The host arrays are the record; the device copies are made
    on first use and after every `add`.  A phase of more than 8 elements cannot be a candidate of any query and is counted in `dropped`."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.nelem, self.Z = np.zeros(0, np.int32), np.zeros((0, MAX_ELEMS), np.int32)
        self.frac, self.energy = np.zeros((0, MAX_ELEMS)), np.zeros(0)
        self.masks = np.zeros((0, 2), np.uint64)
        self.dropped = 0
        self._cache, self._dev = {}, None

    def __len__(self):
        return len(self.nelem)

    def arrays(self):
        return dict(nelem=self.nelem, Z=self.Z, frac=self.frac, energy=self.energy)

    def add_rows(self, Z_lists, fracs, energies):
        """Append rows given as element lists, fraction lists and energies per atom.  Returns the row numbers (-1: more than 8 elements)."""
        out, nel, Zs, Fs, Es, Ms = [], [], [], [], [], []
        for zl, fl, e in zip(Z_lists, fracs, energies):
            zl, fl = np.asarray(zl, np.int64).reshape(-1), np.asarray(fl, np.float64).reshape(-1)
            if len(zl) != len(fl) or len(zl) == 0:
                raise ValueError(f"PhaseBank.add: {len(zl)} elements with {len(fl)} fractions")
            if len(zl) > MAX_ELEMS:
                self.dropped += 1
                out.append(-1)
                continue
            order = np.argsort(zl, kind="stable")
            zl, fl = zl[order], fl[order]
            if (np.diff(zl) <= 0).any() or not np.isfinite(fl).all() or (fl <= 0).any():
                raise ValueError(f"PhaseBank.add: elements {zl.tolist()} with fractions {fl.tolist()}: repeated element, or a fraction that is not positive and finite")
            z8, f8 = np.zeros(MAX_ELEMS, np.int32), np.zeros(MAX_ELEMS)
            z8[:len(zl)], f8[:len(zl)] = zl, fl
            out.append(len(self.nelem) + len(nel))
            nel.append(len(zl)), Zs.append(z8), Fs.append(f8), Es.append(float(e)), Ms.append(element_mask(zl))
        if nel:
            self.nelem = np.concatenate([self.nelem, np.asarray(nel, np.int32)])
            self.Z = np.concatenate([self.Z, np.stack(Zs)])
            self.frac = np.concatenate([self.frac, np.stack(Fs)])
            self.energy = np.concatenate([self.energy, np.asarray(Es, np.float64)])
            self.masks = np.concatenate([self.masks, np.stack(Ms)])
            self._cache, self._dev = {}, None
        return out

    def add(self, records, energies, per_atom=True):
        """Append one row per record; `energies` per atom, or totals with per_atom=False."""
        energies = np.asarray(energies, np.float64).reshape(-1)
        if len(energies) != len(records):
            raise ValueError(f"PhaseBank.add: {len(energies)} energies for {len(records)} records")
        comps = [composition(r) for r in records]
        if any(n == 0 for _, _, n in comps):
            raise ValueError("PhaseBank.add: a record without atoms")
        e = [float(v) if per_atom else float(v) / n for v, (_, _, n) in zip(energies, comps)]
        return self.add_rows([c[0] for c in comps], [c[1] for c in comps], e)

    @classmethod
    def from_records(cls, records, energies, per_atom=True, device="cuda"):
        bank = cls(device)
        bank.add(records, energies, per_atom)
        return bank

    def candidates(self, element_set):
        """The rows whose elements all belong to `element_set` (ascending row numbers, int32): a subset test on the element masks, cached per
        set until the next `add`."""
        key = tuple(sorted(int(z) for z in element_set))
        hit = self._cache.get(key)
        if hit is None:
            outside = ~element_mask(key)
            hit = np.flatnonzero(((self.masks & outside) == 0).all(axis=1)).astype(np.int32) if len(self) else np.zeros(0, np.int32)
            self._cache[key] = hit
        return hit

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, nelem=self.nelem, Z=self.Z, frac=self.frac, energy=self.energy)
        return path

    @classmethod
    def load(cls, path, device="cuda"):
        with np.load(path, allow_pickle=False) as z:
            nelem, Z, frac, energy = z["nelem"].astype(np.int64), z["Z"].astype(np.int64), z["frac"].astype(np.float64), z["energy"].astype(np.float64)
        M = len(nelem)
        if Z.shape != (M, MAX_ELEMS) or frac.shape != (M, MAX_ELEMS) or energy.shape != (M,) or (M and (nelem.min() < 1 or nelem.max() > MAX_ELEMS)):
            raise ValueError(f"PhaseBank.load: {path} is inconsistent ({M} rows, Z {Z.shape}, frac {frac.shape}, energy {energy.shape})")
        bank = cls(device)
        bank.add_rows([Z[i, :nelem[i]] for i in range(M)], [frac[i, :nelem[i]] for i in range(M)], energy)
        return bank

    def device_arrays(self):
        if self.device.type != "cuda":
            raise RuntimeError("the convex-hull solver runs on the GPU: the bank lives on " + str(self.device))
        if self._dev is None:
            pad = lambda a: a if len(a) else np.zeros((1,) + a.shape[1:], a.dtype)   # (a valid pointer for an empty bank)
            self._dev = {k: torch.from_numpy(np.ascontiguousarray(pad(v))).to(self.device) for k, v in self.arrays().items()}
        return self._dev


# ---- the groups ---------------------------------------------------------------------------------------------------------------------------
def build_groups(element_lists, valid, bank):
    """The CSR arrays of one call: a group per element set among the valid records, in order of first appearance; its queries in list order;
    its candidates `bank.candidates(set)`."""
    order, members = [], {}
    for i, zl in enumerate(element_lists):
        if not valid[i]:
            continue
        key = tuple(int(z) for z in zl)
        if key not in members:
            members[key] = []
            order.append(key)
        members[key].append(i)
    G = len(order)
    gZ, q_off, c_off, q_idx, c_idx = np.zeros((G, MAX_ELEMS), np.int32), [0], [0], [], []
    for g, key in enumerate(order):
        gZ[g, :len(key)] = key
        q_idx += members[key]
        c_idx.append(bank.candidates(key))
        q_off.append(len(q_idx))
        c_off.append(c_off[-1] + len(c_idx[-1]))
    i32 = lambda x: np.asarray(x, np.int32).reshape(-1)
    return dict(sets=order, grp_nelem=i32([len(k) for k in order]), grp_Z=gZ, grp_q_off=i32(q_off), q_idx=i32(q_idx), grp_c_off=i32(c_off),
                c_idx=np.concatenate(c_idx).astype(np.int32) if c_idx else np.zeros(0, np.int32))


def empty_result(n):
    return dict(e_hull=np.full(n, np.nan), e_above=np.full(n, np.nan), chempot=np.full((n, MAX_ELEMS), np.nan), decomp_frac=np.zeros((n, MAX_ELEMS)),
                decomp_idx=np.full((n, MAX_ELEMS), -1, np.int64), iters=np.zeros(n, np.int64), status=np.full(n, NOT_RUN, np.int64),
                flags=np.zeros(n, np.int64))


# ---- the kernel call ----------------------------------------------------------------------------------------------------------------------
class _Call:
    """One prepared mi_hull_above call: the argument block and the device arrays it points into (`launch` enqueues, `read` copies back)."""

    def __init__(self, args, keep, fout, iout, Q):
        self.args, self.keep, self.fout, self.iout, self.Q = args, keep, fout, iout, Q

    def launch(self):
        from . import _lib
        _lib.check(_lib.load().mi_hull_above(C.byref(self.args), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "mi_hull_above")

    def read(self):
        Q, f, i = self.Q, self.fout.cpu().numpy(), self.iout.cpu().numpy().astype(np.int64)
        return dict(e_hull=f[:Q].copy(), e_above=f[Q:2 * Q].copy(), chempot=f[2 * Q:10 * Q].reshape(Q, 8).copy(), decomp_frac=f[10 * Q:].reshape(Q, 8).copy(),
                    decomp_idx=i[:8 * Q].reshape(Q, 8), iters=i[8 * Q:9 * Q], status=i[9 * Q:10 * Q], flags=i[10 * Q:])


def prepare_call(bank, groups, query_c, query_e, no_lds=False):
    """The upload and the argument block of one call (None when there is nothing to do): one upload of the integer arrays and one of the
    queries; the outputs pre-filled as `empty_result`, so that a row no group owns stays visible."""
    from . import _lib
    lib = _lib.load()
    dev = bank.device_arrays()
    Q, G = len(query_e), len(groups["grp_nelem"])
    nnz_q, nnz_c = len(groups["q_idx"]), len(groups["c_idx"])
    if Q == 0 or G == 0 or nnz_q == 0:
        return None
    parts = [np.ascontiguousarray(groups[k], np.int32).reshape(-1) for k in ("grp_nelem", "grp_Z", "grp_q_off", "q_idx", "grp_c_off", "c_idx")]
    parts = [p if len(p) else np.zeros(1, np.int32) for p in parts]
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    ints = torch.from_numpy(np.concatenate(parts)).to(bank.device)
    qin = torch.from_numpy(np.concatenate([np.ascontiguousarray(query_c, np.float64).reshape(-1), np.ascontiguousarray(query_e, np.float64).reshape(-1)])).to(bank.device)
    # outputs: doubles e_hull [Q] | e_above [Q] | chempot [Q][8] | decomp_frac [Q][8], then ints decomp_idx [Q][8] | iters | status | flags
    fout = torch.full((18 * Q,), float("nan"), dtype=torch.float64, device=bank.device)
    fout[10 * Q:] = 0.0
    iout = torch.zeros(11 * Q, dtype=torch.int32, device=bank.device)
    iout[:8 * Q] = -1
    iout[9 * Q:10 * Q] = NOT_RUN
    nbytes = int(lib.mi_hull_workspace(G, nnz_q, nnz_c))
    _lib.check(0 if nbytes > 0 else nbytes, "mi_hull_workspace")
    work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=bank.device)
    at = lambda t, k=0: C.c_void_p(t.data_ptr() + t.element_size() * int(k))
    a = _lib.HullArgs()
    a.bank_nelem, a.bank_Z, a.bank_frac, a.bank_energy = at(dev["nelem"]), at(dev["Z"]), at(dev["frac"]), at(dev["energy"])
    a.grp_nelem, a.grp_Z, a.grp_q_off, a.q_idx, a.grp_c_off, a.c_idx = (at(ints, offs[k]) for k in range(6))
    a.query_c, a.query_e, a.workspace = at(qin), at(qin, 8 * Q), at(work)
    a.e_hull, a.e_above, a.chempot, a.decomp_frac = at(fout), at(fout, Q), at(fout, 2 * Q), at(fout, 10 * Q)
    a.decomp_idx, a.iters, a.status, a.flags = at(iout), at(iout, 8 * Q), at(iout, 9 * Q), at(iout, 10 * Q)
    a.M, a.G, a.Q, a.nnz_q, a.nnz_c = len(bank), G, Q, nnz_q, nnz_c
    a.max_elems, a.no_lds = int(min(MAX_ELEMS, max(1, int(np.max(groups["grp_nelem"]))))), 1 if no_lds else 0
    return _Call(a, (dev, ints, qin, work), fout, iout, Q)


def _run_kernel(bank, groups, query_c, query_e, no_lds=False):
    """One mi_hull_above call: the group arrays of `build_groups` (not validated here: the kernel's guard is the last line), query_c
    [Q][8] and query_e [Q] float64.  Two uploads, two launches, one read-back.  Returns the dict of `empty_result`; rows no group owns
    keep its pre-fill."""
    call = prepare_call(bank, groups, query_c, query_e, no_lds)
    if call is None:
        return empty_result(len(query_e))
    call.launch()
    return call.read()


def energy_above_hull(records, energies, bank, per_atom=True, no_lds=False):
    """Per record the energy per atom of the hull of `bank` at its composition (`e_hull`), `e_above` = its own energy per atom minus that
    (negative below the hull: the record is not a member of the bank), the chemical potentials `chempot` [n][8] in the order of the record's
    sorted elements, the decomposition (`decomp_idx` bank rows, `decomp_frac`), the pivot count `iters` and `status`.  Same length and order
    as the input.  A record with more than 8 elements, without atoms or with an energy that is not finite is never dropped: it comes back
    with NaN and status NOT_RUN."""
    n = len(records)
    energies = np.asarray(energies, np.float64).reshape(-1)
    if len(energies) != n:
        raise ValueError(f"energy_above_hull: {len(energies)} energies for {n} records")
    comps = [composition(r) for r in records]
    e_q = np.array([energies[i] if per_atom or comps[i][2] == 0 else energies[i] / comps[i][2] for i in range(n)], np.float64).reshape(n)
    valid = [1 <= len(comps[i][0]) <= MAX_ELEMS and bool(np.isfinite(e_q[i])) for i in range(n)]
    qc = np.zeros((n, MAX_ELEMS))
    for i in range(n):
        if valid[i]:
            qc[i, :len(comps[i][1])] = comps[i][1]
    groups = build_groups([c[0] for c in comps], valid, bank)
    out = _run_kernel(bank, groups, qc, e_q, no_lds) if any(valid) else empty_result(n)
    if np.asarray(out["flags"]).any():
        raise RuntimeError("energy_above_hull: the kernel's guard skipped a candidate that the bank's own subset test had passed")
    out["elements"] = np.zeros((n, MAX_ELEMS), np.int64)
    for i in range(n):
        if len(comps[i][0]) <= MAX_ELEMS:
            out["elements"][i, :len(comps[i][0])] = comps[i][0]
    return out


def stable_mask(result, threshold=STABLE_THRESHOLD):
    """True where the solver ended at an optimum and e_above <= threshold (eV/atom).  NO_TERMINAL, ITER_CAP, UNBOUNDED and a record that was
    not run are not stable."""
    e = np.asarray(result["e_above"], np.float64)
    with np.errstate(invalid="ignore"):
        return (np.asarray(result["status"]) == OK) & np.isfinite(e) & (e <= float(threshold))


class SUNFilter:
    """The reference's filter call shape, `flt(data_list, structures, energies) -> (data, structures, metrics)`, for sample_cfg.filter: keeps
    the crystals that are stable against the phase bank, unique within the batch and novel against the fingerprint bank.  `phase_path`: a
    .npz of scripts/build_phase_bank.py; `reference_path`, `remember`, `fp_tol`, `fp_args`: the `novelty.UNFilter` it owns.  metrics: a
    subset of {"stable", "unique", "novel"}; "validity" is accepted and ignored -- unless `smact` is given (a chemistry.SmactValidity, a path
    or its config mapping): then the composition test runs first on the (relaxed) structures, only the valid ones go on, and
    `valid_frac` is reported (novelty.validity_first).  "stable" needs the energies of sample_cfg.mlip_opt."""

    def __init__(self, metrics=("stable", "unique", "novel"), phase_path=None, reference_path=None, threshold=STABLE_THRESHOLD, per_atom=True,
                 remember=False, fp_tol=None, fp_args=None, device="cuda", bank=None, matcher="fingerprint", ltol=0.2, stol=0.3, angle_tol=5.0, primitive=False, symprec=0.1,
                 smact=None, **ignored):
        from .novelty import UNFilter
        if smact is not None:
            from .chemistry import make_smact
            smact = make_smact(smact)
        self.smact = smact
        from .structure import FP_TOL
        metrics = [str(m) for m in metrics]
        for m in metrics:
            if m == "synthesizable":
                raise ValueError("SUNFilter: metric 'synthesizable' is not built -- it needs a synthesizability model and its downloaded weights")
            if m not in ("stable", "unique", "novel", "validity"):
                raise ValueError(f"SUNFilter: metric {m!r} is none of 'stable', 'unique', 'novel', 'validity'")
        self.metrics = tuple(m for m in ("stable", "unique", "novel") if m in metrics)
        self.validity = "validity" in metrics and self.smact is not None
        if "stable" in self.metrics and phase_path is None and bank is None:
            raise ValueError("SUNFilter: metric 'stable' needs phase_path (a .npz phase bank of scripts/build_phase_bank.py) or bank")
        if not (np.isfinite(threshold)):
            raise ValueError(f"SUNFilter: threshold = {threshold!r} is not finite")
        self.threshold, self.per_atom, self.phase_path, self.device = float(threshold), bool(per_atom), phase_path, device
        self.un = UNFilter(metrics=[m for m in self.metrics if m != "stable"], reference_path=reference_path, remember=remember,
                           fp_tol=FP_TOL if fp_tol is None else fp_tol, fp_args=fp_args, device=device, matcher=matcher, ltol=ltol, stol=stol,
                           angle_tol=angle_tol, primitive=primitive, symprec=symprec)
        self._bank = bank

    @property
    def bank(self):
        if self._bank is None:   # on first use: constructing the filter touches no device
            self._bank = PhaseBank.load(self.phase_path, device=self.device)
        return self._bank

    def __call__(self, data_list, structures, energies=None):
        if not self.validity:
            return self._filter(data_list, structures, energies)
        from .novelty import validity_first
        return validity_first(self.smact, self._filter, data_list, structures, energies)

    def _filter(self, data_list, structures, energies=None):
        from . import novelty
        records = structures if structures is not None else data_list
        n = len(records)
        want_s = "stable" in self.metrics
        if want_s and energies is None:
            raise ValueError("SUNFilter: metric 'stable' needs the energies of a relaxation: set sample_cfg.mlip_opt (relax.Relaxer), "
                             "or drop 'stable' from the metrics")
        un = self.un
        if n == 0:
            m = {"unique_frac": 0.0, "novel_frac": 0.0, "un_frac": 0.0, "bank_size": float(len(un.bank)), "stable_frac": 0.0,
                 "e_above_hull_mean": float("nan"), "no_terminal": 0.0, "sun_frac": 0.0, "phase_bank_size": float(len(self.bank)) if want_s else 0.0}
            return data_list, structures, m
        rms_mean = None
        if un.matcher == "structure":   # the structure matcher's U and N
            uniq, novel, rms_mean = un.structure_masks(records)
        else:
            fingerprints = novelty._fingerprints_of(records, None, un.bank.fp_args)
            uniq = novelty.unique_mask(records, fingerprints, un.fp_tol, un.bank.fp_args, un.device)
            novel = novelty.novel_mask(records, un.bank, fingerprints)
        if want_s:
            res = energy_above_hull(records, energies, self.bank, self.per_atom)
            stable = stable_mask(res, self.threshold)
            fin = np.isfinite(res["e_above"])
            e_mean = float(res["e_above"][fin].mean()) if fin.any() else float("nan")
            no_term = float((res["status"] == NO_TERMINAL).sum())
        else:
            res, stable, e_mean, no_term = None, np.ones(n, bool), float("nan"), 0.0
        self.last_result = res
        keep = np.ones(n, bool)
        for name, mask in (("stable", stable), ("unique", uniq), ("novel", novel)):
            if name in self.metrics:
                keep &= mask
        idx = [i for i in range(n) if keep[i]]
        if un.remember and idx and un.matcher == "structure":
            un.bank.add([records[i] for i in idx])
        elif un.remember and idx:
            un.bank.add([records[i] for i in idx], (fingerprints[0][idx], fingerprints[1][idx]))
        metrics = {"unique_frac": float(uniq.mean()), "novel_frac": float(novel.mean()), "un_frac": float((uniq & novel).mean()),
                   "bank_size": float(len(un.bank)), "stable_frac": float(stable.mean()) if want_s else float("nan"), "e_above_hull_mean": e_mean,
                   "no_terminal": no_term, "sun_frac": float((stable & uniq & novel).mean()),
                   "phase_bank_size": float(len(self.bank)) if want_s else 0.0}
        if rms_mean is not None:
            metrics["match_rms_mean"] = rms_mean
        pick = lambda xs: [xs[i] for i in idx] if xs is not None else None
        return pick(data_list), pick(structures), metrics
