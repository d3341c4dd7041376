"""Substrate matching on the device (include/matinvent_hip_zsl.h): the minimal coincident interface area (MCIA) between films
and a bank of substrates by Zur-McGill superlattices -- the reference's `calc_mcia` (rewards/calculators/pymatgen/calc.py), which runs
pymatgen's SubstrateAnalyzer over ZSLGenerator.  A stated restatement: pymatgen is absent, so every pymatgen detail is
[UPSTREAM-UNVERIFIED] and agreement with it is unverified; the closed forms and the brute force of tests/zsl_ref64.py are the ground truth.
Planes are indexed in the cell as given (no conventional standard cell, no symmetry reduction of the plane list): for centred lattices
the plane set of film_max_miller = 1 differs from the reference's, and film_max_miller = 2 is the way to cover them.  Not built: slab
terminations, the elastic-energy term, bidirectional matching."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .structure import lattice_matrix

STATUS = ("OK", "NO_MATCH", "MULT_CAP", "REDUCE_CAP", "BAD_CELL")
ITEM_CAP = 1 << 22   # items per search launch: the item rows of a chunk of films (168 bytes each)


def miller_planes(m=1):
    """(h, k, l) in [-m, m]^3, not all zero, gcd 1, the first non-zero entry positive, in ascending lexicographic order (13 at m = 1)."""
    m = int(m)
    if not 1 <= m <= 3:
        raise ValueError(f"max_miller = {m}: 1 .. 3")
    out = []
    for h in range(-m, m + 1):
        for k in range(-m, m + 1):
            for l in range(-m, m + 1):
                nz = [v for v in (h, k, l) if v != 0]
                if nz and nz[0] > 0 and math.gcd(math.gcd(abs(h), abs(k)), abs(l)) == 1:
                    out.append((h, k, l))
    return out


def cell_matrix(cell):
    """3 x 3 float32 rows from six parameters (a, b, c, alpha, beta, gamma), a 3 x 3 matrix, a record with lengths and angles, or the first
    frame of a file structure.read_extxyz reads."""
    if isinstance(cell, str):
        from .structure import read_extxyz
        return np.asarray(read_extxyz(cell)[0].lattice, np.float64).astype(np.float32)
    if hasattr(cell, "lengths") and hasattr(cell, "angles"):
        lengths, angles = np.asarray(cell.lengths, np.float64).reshape(-1), np.asarray(cell.angles, np.float64).reshape(-1)
        return lattice_matrix(lengths, angles).astype(np.float32)
    arr = np.asarray(cell, np.float64)
    if arr.shape == (6,):
        return lattice_matrix(arr[:3], arr[3:]).astype(np.float32)
    if arr.size == 9:
        return arr.reshape(3, 3).astype(np.float32)
    raise ValueError(f"a cell is six parameters, a 3 x 3 matrix, a record or a file; got shape {arr.shape}")


class Substrate:
    """A named cell and, optionally, its explicit plane list (the reference uses (1, 0, 0) for Si, GaAs and InP); without one the planes
    are miller_planes(substrate_max_miller)."""

    def __init__(self, name, cell, millers=None):
        self.name, self.cell = str(name), cell_matrix(cell)
        self.millers = None
        if millers is not None:
            ms = [tuple(int(v) for v in hkl) for hkl in millers]
            if not ms or any(len(hkl) != 3 or not any(hkl) or max(abs(v) for v in hkl) > _lib.ZSL_MAX_MILLER for hkl in ms):
                raise ValueError(f"substrate {name!r}: millers = {millers!r}: non-zero integer triples within +-{_lib.ZSL_MAX_MILLER}")
            self.millers = ms

    def planes(self, max_miller):
        return self.millers if self.millers is not None else miller_planes(max_miller)


def as_substrate(substrate):
    return substrate if isinstance(substrate, Substrate) else Substrate("substrate", substrate)


class ZSL:
    """The parameters of the search; the defaults are the reference's (SubstrateAnalyzer(film_max_miller=1, substrate_max_miller=1))."""

    def __init__(self, max_area=400.0, max_area_ratio_tol=0.09, max_length_tol=0.03, max_angle_tol=0.01, film_max_miller=1, substrate_max_miller=1):
        self.max_area, self.max_area_ratio_tol, self.max_length_tol, self.max_angle_tol = (float(v) for v in (max_area, max_area_ratio_tol, max_length_tol, max_angle_tol))
        self.film_max_miller, self.substrate_max_miller = int(film_max_miller), int(substrate_max_miller)
        if not (self.max_area > 0.0 and math.isfinite(self.max_area)):
            raise ValueError(f"max_area = {max_area}: positive and finite")
        for k in ("max_area_ratio_tol", "max_length_tol", "max_angle_tol"):
            if not (getattr(self, k) >= 0.0 and math.isfinite(getattr(self, k))):
                raise ValueError(f"{k} = {getattr(self, k)}: non-negative and finite")
        miller_planes(self.film_max_miller), miller_planes(self.substrate_max_miller)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def plane_arrays(lat, hkl, cell_of, max_area, fill=None):
    """mi_zsl_planes on device tensors: lat [C, 9] float32, hkl [P, 3] int32, cell_of [P] int32 or None (every cell takes every plane):
    (vec [T, 6], area [T], mult [T], status [T])."""
    lib = _lib.load()
    dev = lat.device
    Cn, P = lat.shape[0], hkl.shape[0]
    T = P if cell_of is not None else Cn * P
    z = (lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)) if fill is None else fill
    vec, area, mult, status = z((T, 6), torch.float64), z((T,), torch.float64), z((T,), torch.int32), z((T,), torch.int32)
    args = _lib.ZslPlanesArgs(lat.data_ptr(), hkl.data_ptr(), cell_of.data_ptr() if cell_of is not None else None, Cn, P, float(max_area), vec.data_ptr(),
                              area.data_ptr(), mult.data_ptr(), status.data_ptr())
    _lib.check(lib.mi_zsl_planes(C.byref(args), _stream()), "mi_zsl_planes")
    return vec, area, mult, status


class SubstrateBank:
    """The substrates' planes and superlattice tables, built once and kept on the device; `save` / `load` as .npz of data only."""

    FIELDS = ("lat", "hkl", "cell_of", "sub_off", "vec", "area", "mult", "status", "table")

    def __init__(self, substrates, zsl=None, device="cuda", fill=None):
        zsl = zsl or ZSL()
        subs = [as_substrate(s) for s in (substrates if isinstance(substrates, (list, tuple)) else [substrates])]
        if not subs:
            raise ValueError("a bank needs at least one substrate")
        self.names, self.max_area, self.device = [s.name for s in subs], zsl.max_area, torch.device(device)
        planes = [s.planes(zsl.substrate_max_miller) for s in subs]
        put = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.device)
        self.lat = put(np.stack([s.cell.reshape(9) for s in subs]), np.float32)
        self.hkl = put(np.array([hkl for ps in planes for hkl in ps]).reshape(-1, 3), np.int32)
        self.cell_of = put(np.array([k for k, ps in enumerate(planes) for _ in ps]), np.int32)
        self.sub_off = put(np.cumsum([0] + [len(ps) for ps in planes]), np.int32)
        self.vec, self.area, self.mult, self.status = plane_arrays(self.lat, self.hkl, self.cell_of, zsl.max_area, fill)
        lib = _lib.load()
        nbytes = lib.mi_zsl_workspace(self.Ps)
        assert nbytes == self.Ps * _lib.ZSL_TABLE * 24
        self.table = torch.zeros((self.Ps, _lib.ZSL_TABLE, 3), dtype=torch.float64, device=self.device)
        _lib.check(lib.mi_zsl_tables(self.vec.data_ptr(), self.mult.data_ptr(), self.status.data_ptr(), self.Ps, self.table.data_ptr(), _stream()), "mi_zsl_tables")

    @property
    def Ps(self):
        return int(self.hkl.shape[0])

    @property
    def S(self):
        return len(self.names)

    def save(self, path):
        np.savez(path, names=np.array(self.names), max_area=np.float64(self.max_area), **{k: getattr(self, k).cpu().numpy() for k in self.FIELDS})
        return path

    @classmethod
    def load(cls, path, device="cuda"):
        self = cls.__new__(cls)
        with np.load(path, allow_pickle=False) as f:
            self.names, self.max_area, self.device = [str(n) for n in f["names"]], float(f["max_area"]), torch.device(device)
            for k in cls.FIELDS:
                setattr(self, k, torch.from_numpy(f[k]).to(self.device))
        if self.table.shape != (self.Ps, _lib.ZSL_TABLE, 3) or self.sub_off.numel() != self.S + 1:
            raise ValueError(f"{path}: not a bank of this build (table {tuple(self.table.shape)})")
        return self


ROW_I = ("status", "film_plane", "n_f", "n_s")


class MatchResult:
    """The arrays of mi_zsl_reduce on the device (res_d [B, Ps, 10], res_i [B, Ps, 20], res_n [B, Ps]; mcia, mcia_plane, mcia_status
    [B, S]) and, read once in one transfer, their named views as numpy: per (film, substrate plane) `area`, `status`, `film_plane`, `n_f`,
    `n_s`, `film_hnf`, `sub_hnf` [.., 3] = (i, j, n / i), `strains` [.., 3], `n_matches`, and `least_strained` (a dict of the same names
    plus `strain`); per (film, substrate) `mcia`, `mcia_plane`, `mcia_status`."""

    def __init__(self, res_d, res_i, res_n, mcia, mcia_plane, mcia_status, film_hkl, bank, count):
        self.res_d, self.res_i, self.res_n, self.d_mcia, self.d_mcia_plane, self.d_mcia_status = res_d, res_i, res_n, mcia, mcia_plane, mcia_status
        self.film_hkl, self.bank, self.count = film_hkl, bank, bool(count)
        self._host = None

    def __len__(self):
        return int(self.res_d.shape[0])

    def host(self):
        if self._host is None:
            parts = (self.res_d, self.res_i, self.res_n, self.d_mcia, self.d_mcia_plane, self.d_mcia_status)
            raw = torch.cat([t.contiguous().view(-1).view(torch.uint8) for t in parts]).cpu().numpy()   # the one read
            out, at = [], 0
            for t in parts:
                n = t.numel() * t.element_size()
                out.append(raw[at:at + n].view({torch.float64: np.float64, torch.int32: np.int32, torch.int64: np.int64}[t.dtype]).reshape(tuple(t.shape)))
                at += n
            self._host = out
        return self._host

    @staticmethod
    def _match(d, r):
        return dict(area=d[..., 0].copy(), strains=d[..., 1:4].copy(), film_plane=r[..., 0].copy(), n_f=r[..., 1].copy(), n_s=r[..., 2].copy(),
                    film_hnf=r[..., 3:6].copy(), sub_hnf=r[..., 6:9].copy())

    def __getattr__(self, name):
        if name.startswith("_") or name in ("res_d", "res_i", "res_n"):
            raise AttributeError(name)
        d, r, n, mcia, plane, status = self.host()
        if name == "status":
            return r[..., 0].copy()
        if name == "n_matches":
            return n.copy()
        if name == "least_strained":
            return dict(self._match(d[..., 5:9], r[..., 10:19]), strain=d[..., 4].copy())
        if name in ("mcia", "mcia_plane", "mcia_status"):
            return dict(mcia=mcia, mcia_plane=plane, mcia_status=status)[name].copy()
        low = self._match(d[..., 0:4], r[..., 1:10])
        if name in low:
            return low[name]
        raise AttributeError(name)


def match_arrays(zsl, lat, bank, count=False, fill=None):
    """planes -> search -> reduce on device tensors: lat [B, 9] float32 (cell rows) against a SubstrateBank; nothing is read back.  `fill`
    builds the output tensors and the item rows (tests poison them)."""
    lib = _lib.load()
    if abs(bank.max_area - zsl.max_area) > 0.0:
        raise ValueError(f"the bank's tables were built for max_area = {bank.max_area}, the search asks for {zsl.max_area}")
    lat = lat.to(torch.float32).reshape(-1, 9).contiguous()
    dev = lat.device
    B, Ps, S = int(lat.shape[0]), bank.Ps, bank.S
    hkl_list = miller_planes(zsl.film_max_miller)
    hkl = torch.tensor(hkl_list, dtype=torch.int32, device=dev)
    Pf = len(hkl_list)
    z = (lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)) if fill is None else fill
    res = MatchResult(z((B, Ps, _lib.ZSL_ROW_D), torch.float64), z((B, Ps, _lib.ZSL_ROW_I), torch.int32), z((B, Ps), torch.int64), z((B, S), torch.float64),
                      z((B, S), torch.int32), z((B, S), torch.int32), hkl_list, bank, count)
    if B == 0:
        return res
    vec, area, mult, status = plane_arrays(lat, hkl, None, zsl.max_area, fill)
    res.planes = (vec, area, mult, status)
    step = max(1, ITEM_CAP // (Pf * Ps))
    rows = min(step, B) * Pf * Ps
    item_d, item_i, item_n = z((rows, _lib.ZSL_ROW_D), torch.float64), z((rows, _lib.ZSL_ROW_I), torch.int32), z((rows,), torch.int64)
    p = lambda t: t.data_ptr()
    for b0 in range(0, B, step):
        nb = min(step, B - b0)
        f0 = b0 * Pf
        sa = _lib.ZslSearchArgs(p(vec[f0:]), p(area[f0:]), p(mult[f0:]), p(status[f0:]), p(bank.area), p(bank.mult), p(bank.status), p(bank.table), nb, Pf, Ps,
                                1 if count else 0, zsl.max_area_ratio_tol, zsl.max_length_tol, zsl.max_angle_tol, p(item_d), p(item_i), p(item_n))
        _lib.check(lib.mi_zsl_search(C.byref(sa), _stream()), "mi_zsl_search")
        ra = _lib.ZslReduceArgs(p(item_d), p(item_i), p(item_n), p(bank.sub_off), nb, Pf, Ps, S, 1 if count else 0, p(res.res_d[b0:]), p(res.res_i[b0:]),
                                p(res.res_n[b0:]), p(res.d_mcia[b0:]), p(res.d_mcia_plane[b0:]), p(res.d_mcia_status[b0:]))
        _lib.check(lib.mi_zsl_reduce(C.byref(ra), _stream()), "mi_zsl_reduce")
    return res


def record_cells(records):
    """[B, 9] float32 cell rows of host records (SimpleStructure / CrystalData-like); a record without a usable cell gets NaN rows, which
    the device flags BAD_CELL -- nothing is dropped or reordered."""
    out = np.full((len(records), 9), np.nan, np.float32)
    for k, r in enumerate(records):
        try:
            out[k] = cell_matrix(r).reshape(9)
        except Exception:
            pass
    return out


def _has_atoms(r):
    return hasattr(r, "lengths") and (hasattr(r, "species") or hasattr(r, "atom_types"))


def match_records(zsl, records, bank, count=False, primitive=False, device=None, conventional=False):
    """The MatchResult of host records against a bank: one upload, the launches, one read at the end (MatchResult.host).  Never drops or
    reorders records.  primitive=True runs symmetry.primitive_records on the films first (a record it cannot analyse keeps its cell);
    conventional=True runs symmetry.conventional_records on them instead, so that the planes are indexed in the conventional
    cell whatever cell the film arrived in.  The two exclude each other."""
    if primitive and conventional:
        raise ValueError("match_records: primitive=True and conventional=True exclude each other: the planes are indexed in one cell")
    dev = torch.device(device) if device is not None else bank.device
    records = list(records)
    if conventional and records:
        from . import symmetry
        good = [k for k, r in enumerate(records) if _has_atoms(r)]
        conv, _ = symmetry.conventional_records([records[k] for k in good], device=dev)
        for k, s in zip(good, conv):
            records[k] = s
    if primitive and records:
        from . import symmetry
        good = [k for k, r in enumerate(records) if hasattr(r, "lengths") and (hasattr(r, "species") or hasattr(r, "atom_types"))]
        prim, _ = symmetry.primitive_records([records[k] for k in good], device=dev)
        for k, s in zip(good, prim):
            records[k] = s
    res = match_arrays(zsl, torch.from_numpy(record_cells(records)).to(dev), bank, count)
    res.host()
    return res


def mcia(records, substrate, zsl=None, primitive=False, device="cuda", conventional=False):
    """The one-substrate shortcut: (mcia [B] in A^2, +inf where nothing matches; status [B]) of the records on one substrate.  With
    conventional=True a substrate given as a record with atoms is put into its conventional cell like the films; a bare cell, a Substrate
    or a bank is taken as given."""
    if primitive and conventional:
        raise ValueError("mcia: primitive=True and conventional=True exclude each other: the planes are indexed in one cell")
    zsl = zsl or ZSL()
    if conventional and _has_atoms(substrate):
        from . import symmetry
        substrate = symmetry.conventional_records([substrate], device=device)[0][0]
    bank = substrate if isinstance(substrate, SubstrateBank) else SubstrateBank([substrate], zsl, device)
    res = match_records(zsl, records, bank, primitive=primitive, device=device, conventional=conventional)
    return res.mcia[:, 0], res.mcia_status[:, 0]
