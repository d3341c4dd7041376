"""Composition validity on the device: charge neutrality and the Pauling test (include/matinvent_hip_chem.h).

The composition half of the reference's `invalid_filter` (pipeline/filters/opt_filter.py:51-52 and :179-180 AND mattergen's
`is_smact_valid` into the pre-filter and again behind the relaxation).  SMACT and its element database are not part of this build and no
table is shipped: the user supplies the data as a JSON file (`ElementTable.load`, written by scripts/build_element_table.py) and this
module ships the algorithm -- the build's own stated rule, every detail of SMACT's and mattergen's marked [UPSTREAM-UNVERIFIED] in the
header.  The enumeration of up to `max_combos` oxidation-state combinations per composition is three launches of `mi_chem_validity`;
nothing here enumerates on the host.

    table = ElementTable.load("elements.json")
    res = validity(records, table)                  # a ValidityResult: valid, status, first, first_ox, atom_ox, ...
    v = SmactValidity("elements.json")              # a callable: records -> bool mask (filters.invalid_filter(..., smact=v))
"""
import ctypes as C
import json
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib

SYMBOLS = ("X H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y Zr Nb Mo Tc "
           "Ru Rh Pd Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir Pt Au Hg Tl Pb Bi "
           "Po At Rn Fr Ra Ac Th Pa U Np Pu Am Cm Bk Cf Es Fm Md No Lr Rf Db Sg Bh Hs Mt Ds Rg Cn Nh Fl Mc Lv Ts Og").split()
assert len(SYMBOLS) == _lib.CHEM_MAX_Z + 1
Z_OF = {s: z for z, s in enumerate(SYMBOLS) if z}

MAX_Z, MAX_STATES, MAX_ELEMS, CHUNK, MAX_BATCH = _lib.CHEM_MAX_Z, _lib.CHEM_MAX_STATES, _lib.CHEM_MAX_ELEMS, _lib.CHEM_CHUNK, _lib.CHEM_MAX_BATCH
DEFAULT_MAX_COMBOS = _lib.CHEM_DEFAULT_MAX_COMBOS
STATUS_NAMES = ("ENUMERATED", "ELEMENTAL", "ALLOY", "BAD_INPUT", "TOO_MANY_ELEMENTS", "UNKNOWN_ELEMENT", "NO_STATES", "TOO_MANY_COMBOS")
(ENUMERATED, ELEMENTAL, ALLOY, BAD_INPUT, TOO_MANY_ELEMENTS, UNKNOWN_ELEMENT, NO_STATES, TOO_MANY_COMBOS) = range(8)


class ElementTable:
    """Per atomic number 1 .. 118: present, the ordered oxidation states, the dense rank of the Pauling electronegativity (ranked here from
    float64 values, equal values share a rank, -1: missing), is_metal -- and the crustal abundance for rewards.PyMatGen (host only).

    `elements`: {symbol: {"ox": [ints], "eneg": float | None, "metal": bool, "abundance": float | None}}; missing keys read as [], None,
    False, None."""

    def __init__(self, elements: dict):
        self.present = np.zeros(MAX_Z + 1, np.int32)
        self.n_states = np.zeros(MAX_Z + 1, np.int32)
        self.ox = np.zeros((MAX_Z + 1, MAX_STATES), np.int32)
        self.eneg_rank = np.full(MAX_Z + 1, -1, np.int32)
        self.is_metal = np.zeros(MAX_Z + 1, np.int32)
        self.eneg = np.full(MAX_Z + 1, np.nan, np.float64)
        self.abundance = np.full(MAX_Z + 1, np.nan, np.float64)
        if not isinstance(elements, dict):
            raise ValueError("ElementTable: `elements` must map element symbols to their rows")
        for sym, row in elements.items():
            if sym not in Z_OF:
                raise ValueError(f"ElementTable: unknown symbol {sym!r}")
            if not isinstance(row, dict):
                raise ValueError(f"ElementTable: {sym}: the row must be a mapping with the keys ox / eneg / metal / abundance")
            unknown = set(row) - {"ox", "eneg", "metal", "abundance"}
            if unknown:
                raise ValueError(f"ElementTable: {sym}: unknown key(s) {sorted(unknown)}")
            z = Z_OF[sym]
            ox = list(row.get("ox") or [])
            if len(ox) > MAX_STATES:
                raise ValueError(f"ElementTable: {sym}: {len(ox)} oxidation states, the list is longer than {MAX_STATES}")
            for o in ox:
                if isinstance(o, bool) or not isinstance(o, (int, np.integer)):
                    raise ValueError(f"ElementTable: {sym}: oxidation state {o!r} is not an integer")
                if not -127 <= int(o) <= 127:
                    raise ValueError(f"ElementTable: {sym}: oxidation state {o} is out of range -127..127")
            if len(set(int(o) for o in ox)) != len(ox):
                raise ValueError(f"ElementTable: {sym}: duplicate oxidation state in {ox}")
            eneg = row.get("eneg")
            if eneg is not None:
                eneg = float(eneg)
                if not math.isfinite(eneg):
                    raise ValueError(f"ElementTable: {sym}: non-finite eneg {eneg}")
                self.eneg[z] = eneg
            ab = row.get("abundance")
            if ab is not None:
                self.abundance[z] = float(ab)
            self.present[z] = 1
            self.n_states[z] = len(ox)
            self.ox[z, :len(ox)] = [int(o) for o in ox]
            self.is_metal[z] = 1 if row.get("metal") else 0
        have = np.isfinite(self.eneg)
        levels = np.unique(self.eneg[have])   # float64, ascending: the device compares these ranks only
        self.eneg_rank[have] = np.searchsorted(levels, self.eneg[have]).astype(np.int32)
        self._device = {}

    @classmethod
    def from_dict(cls, d: dict) -> "ElementTable":
        if not isinstance(d, dict) or "elements" not in d:
            raise ValueError('ElementTable: expected {"elements": {symbol: {...}}}')
        return cls(d["elements"])

    @classmethod
    def load(cls, path: str) -> "ElementTable":
        with open(path) as f:
            return cls.from_dict(json.load(f))

    def to(self, device) -> dict:
        """The five device arrays of mi_chem_args (built once per device)."""
        device = torch.device(device)
        key = str(device)
        if key not in self._device:
            self._device[key] = {k: torch.from_numpy(np.ascontiguousarray(getattr(self, k))).to(device)
                                 for k in ("present", "n_states", "ox", "eneg_rank", "is_metal")}
        return self._device[key]


@dataclass
class ValidityResult:
    """Every output of mi_chem_validity as numpy arrays, rows in the order of the input."""
    valid: np.ndarray        # [B] bool
    status: np.ndarray       # [B] int32 (STATUS_NAMES)
    n_elems: np.ndarray      # [B] int32
    elems: np.ndarray        # [B, 8] int32
    counts: np.ndarray       # [B, 8] int32
    n_combos: np.ndarray     # [B] int64
    n_neutral: np.ndarray    # [B] int64
    n_valid: np.ndarray      # [B] int64
    first: np.ndarray        # [B] int64
    first_ox: np.ndarray     # [B, 8] int32
    atom_ox: np.ndarray      # [N] int32
    num_atoms: np.ndarray    # [B] int64

    def __len__(self):
        return len(self.valid)

    def status_names(self):
        return [STATUS_NAMES[int(s)] for s in self.status]


_OUT = (("valid", 1, torch.int32), ("status", 1, torch.int32), ("n_elems", 1, torch.int32), ("elems", MAX_ELEMS, torch.int32), ("counts", MAX_ELEMS, torch.int32),
        ("n_combos", 1, torch.int64), ("n_neutral", 1, torch.int64), ("n_valid", 1, torch.int64), ("first", 1, torch.int64), ("first_ox", MAX_ELEMS, torch.int32))


def _species_of(rec):
    if hasattr(rec, "species"):
        return [int(z) for z in rec.species]
    return [int(z) for z in rec.atom_types.reshape(-1).tolist()]


def _inputs(records, device):
    """(num_atoms [B] int64, atom_types [N] int32) on `device` from records or from a (num_atoms, atom_types) pair of tensors / arrays."""
    if isinstance(records, tuple) and len(records) == 2:
        na, at = records
        na = torch.as_tensor(na).reshape(-1).to(device=device, dtype=torch.int64)
        at = torch.as_tensor(at).reshape(-1).to(device=device, dtype=torch.int32)
        return na, at
    species = [_species_of(r) for r in records]
    na = torch.tensor([len(s) for s in species], dtype=torch.int64)
    at = torch.tensor([z for s in species for z in s], dtype=torch.int32)
    return na.to(device), at.to(device)


class ValidityCall:
    """One prepared batch: `launch` enqueues the mi_chem_validity calls (MAX_BATCH crystals each) on the current stream, `read` makes the
    one copy back.  `poison` pre-fills every output (tests)."""

    def __init__(self, records, table: ElementTable, use_pauling_test=True, include_alloys=True, max_combos=DEFAULT_MAX_COMBOS, device=None,
                 poison: Optional[int] = None):
        if not isinstance(table, ElementTable):
            raise TypeError("validity: `table` must be an ElementTable (ElementTable.load(path))")
        max_combos = int(max_combos)
        if not 1 <= max_combos <= MAX_STATES ** MAX_ELEMS:
            raise ValueError(f"validity: max_combos = {max_combos} outside 1..{MAX_STATES}^{MAX_ELEMS}")
        if device is None:
            device = records[1].device if isinstance(records, tuple) and isinstance(records[1], torch.Tensor) and records[1].is_cuda else "cuda"
        self.device = torch.device(device)
        self.table, self.max_combos = table, max_combos
        self.use_pauling_test, self.include_alloys = bool(use_pauling_test), bool(include_alloys)
        self.num_atoms, self.atom_types = _inputs(records, self.device)
        self.B, self.N = int(self.num_atoms.numel()), int(self.atom_types.numel())
        # the offsets are formed on the device from the counts: a batch that arrives on the device is never read back for them
        self.node_off = torch.zeros(self.B + 1, dtype=torch.int64, device=self.device)
        self.node_off[1:] = torch.cumsum(self.num_atoms, 0)
        self.node_off = self.node_off.clamp(-1, 2 ** 31 - 1).to(torch.int32)
        fill = 0 if poison is None else int(poison)
        self.out = {k: torch.full((self.B, w) if w > 1 else (self.B,), fill, dtype=dt, device=self.device) for k, w, dt in _OUT}
        self.out["atom_ox"] = torch.full((self.N,), fill, dtype=torch.int32, device=self.device)
        self.calls = []
        if self.B == 0:
            return
        lib = _lib.load()
        tab = table.to(self.device)
        at = lambda t, k=0: C.c_void_p(t.data_ptr() + t.element_size() * int(k))
        for b0 in range(0, self.B, MAX_BATCH):
            nb = min(MAX_BATCH, self.B - b0)
            nbytes = int(lib.mi_chem_workspace(nb, max_combos))
            _lib.check(0 if nbytes > 0 else nbytes, "mi_chem_workspace")
            work = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            a = _lib.ChemArgs()
            a.present, a.n_states, a.ox, a.eneg_rank, a.is_metal = (at(tab[k]) for k in ("present", "n_states", "ox", "eneg_rank", "is_metal"))
            a.node_off, a.atom_types, a.workspace = at(self.node_off, b0), at(self.atom_types), at(work)
            for k, w, _ in _OUT:
                setattr(a, k, at(self.out[k], b0 * w))
            a.atom_ox = at(self.out["atom_ox"])
            a.max_combos, a.B, a.N = max_combos, nb, self.N
            a.use_pauling_test, a.include_alloys = int(self.use_pauling_test), int(self.include_alloys)
            self.calls.append((a, work))

    def launch(self):
        lib = _lib.load()
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        for a, _ in self.calls:
            _lib.check(lib.mi_chem_validity(C.byref(a), stream), "mi_chem_validity")
        return self

    def read(self) -> ValidityResult:
        """One copy back: every output and the atom counts packed into one int64 buffer."""
        parts = [self.out[k].reshape(-1).to(torch.int64) for k, _, _ in _OUT] + [self.out["atom_ox"].to(torch.int64), self.num_atoms]
        flat = torch.cat(parts).cpu().numpy()
        pos, got = 0, {}
        for k, w, dt in _OUT:
            n = self.B * w
            got[k] = flat[pos:pos + n].astype(np.int64 if dt == torch.int64 else np.int32).reshape((self.B, w) if w > 1 else (self.B,))
            pos += n
        got["atom_ox"] = flat[pos:pos + self.N].astype(np.int32)
        got["num_atoms"] = flat[pos + self.N:].astype(np.int64)
        got["valid"] = got["valid"] == 1
        return ValidityResult(**got)


def validity(records, table: ElementTable, use_pauling_test=True, include_alloys=True, max_combos=DEFAULT_MAX_COMBOS, device=None) -> ValidityResult:
    """Charge neutrality and the Pauling test of every record (or of a `(num_atoms, atom_types)` pair), on the device; one read at the
    end; records are never dropped or reordered."""
    return ValidityCall(records, table, use_pauling_test, include_alloys, max_combos, device).launch().read()


class SmactValidity:
    """`v(records) -> bool mask`, the composition half of `invalid_filter`.  `table`: an ElementTable, a path to its JSON file, or the
    mapping {table, use_pauling_test, include_alloys, max_combos} of a config.  The device table is built on first use."""

    KEYS = ("table", "use_pauling_test", "include_alloys", "max_combos")

    def __init__(self, table, use_pauling_test=True, include_alloys=True, max_combos=DEFAULT_MAX_COMBOS, device=None):
        if not isinstance(table, (ElementTable, str)) and hasattr(table, "keys"):
            cfg = dict(table)
            unknown = set(cfg) - set(self.KEYS)
            if unknown or "table" not in cfg:
                raise ValueError(f"SmactValidity: expected the keys {self.KEYS} with `table` set, got {sorted(cfg)}")
            table = cfg["table"]
            use_pauling_test = cfg.get("use_pauling_test", use_pauling_test)
            include_alloys = cfg.get("include_alloys", include_alloys)
            max_combos = cfg.get("max_combos", max_combos)
        if not isinstance(table, (ElementTable, str)):
            raise TypeError(f"SmactValidity: `table` must be an ElementTable or the path of its JSON file, not {table!r} (no table is shipped: "
                            "scripts/build_element_table.py writes one from your data)")
        max_combos = int(max_combos)
        if not 1 <= max_combos <= MAX_STATES ** MAX_ELEMS:
            raise ValueError(f"SmactValidity: max_combos = {max_combos} outside 1..{MAX_STATES}^{MAX_ELEMS}")
        self._table = table
        self.use_pauling_test, self.include_alloys, self.max_combos, self.device = bool(use_pauling_test), bool(include_alloys), max_combos, device
        self.last = None   # the ValidityResult of the latest call

    @property
    def table(self) -> ElementTable:
        if isinstance(self._table, str):
            self._table = ElementTable.load(self._table)
        return self._table

    def result(self, records) -> ValidityResult:
        self.last = validity(records, self.table, self.use_pauling_test, self.include_alloys, self.max_combos, self.device)
        return self.last

    def __call__(self, records) -> np.ndarray:
        if not isinstance(records, tuple) and len(records) == 0:
            return np.zeros(0, dtype=bool)
        return self.result(records).valid.copy()


def make_smact(cfg):
    """None, a SmactValidity, a path or a config mapping -> None or a SmactValidity (the pipelines' `sample_cfg.smact`)."""
    if cfg is None or isinstance(cfg, SmactValidity):
        return cfg
    return SmactValidity(cfg)
