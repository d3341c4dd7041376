"""Space-group operations, point group and primitive cell on the device (include/matinvent_hip_sym.h): the structure matcher
run on (b, b) with a rigid metric, a nearest-atom test and every accepted (map, translation) item kept.  symprec = 0.1 A is the
reference's value (SpacegroupAnalyzer(symprec=0.1)); angle_tol = 5 degrees is the matcher's and is untuned -- spglib's own lattice rule is
[UPSTREAM-UNVERIFIED] and is not reproduced, and agreement with spglib is unverified (it is absent here).  Not built: the space-group
number or Hall symbol, Wyckoff letters, symmetry reduction of the vibration or elastic displacement sets, magnetic and disordered
structures.

The conventional cell (include/matinvent_hip_sym_conv.h): conventional_arrays / conventional_records reduce every crystal to
its primitive cell, analyse that again and build the conventional basis, the centring and the Bravais lattice from the rotation parts.
The rules are this build's own; pymatgen's get_conventional_standard_structure and spglib's standardisation are [UPSTREAM-UNVERIFIED]
(both are absent here) and are not claimed to be reproduced beyond them.

The refined structure (include/matinvent_hip_sym_refine.h): refine_arrays / refined_records project the coordinates and the cell
of every crystal onto the group found at symprec and return the site orbits, their multiplicities and the orders of the site-symmetry
groups; symmetry_primitive_records stands where the reference's get_symmetry_primitive does."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from . import matching
from .structure import record_arrays

SYMPREC, ANGLE_TOL = 0.1, 5.0
CLASSES = (-6, -4, -3, -2, -1, 1, 2, 3, 4, 6)
POINT_GROUPS = ("", "1", "-1", "2", "m", "2/m", "222", "mm2", "mmm", "4", "-4", "4/m", "422", "4mm", "-42m", "4/mmm", "3", "-3", "32", "3m", "-3m", "6", "-6",
                "6/m", "622", "6mm", "-6m2", "6/mmm", "23", "m-3", "432", "-43m", "m-3m")
CRYSTAL_SYSTEMS = ("", "triclinic", "monoclinic", "orthorhombic", "tetragonal", "trigonal", "hexagonal", "cubic")
INFO = ("n_ops", "n_trans", "n_maps", "pg_order", "pg_index", "crystal_system", "has_inversion", "status")
BRAVAIS = ("", "aP", "mP", "mS", "oP", "oS", "oI", "oF", "tP", "tI", "hR", "hP", "cP", "cI", "cF")
CENTRINGS = ("", "P", "A", "B", "C", "I", "F", "R")
CONV_INFO = ("bravais", "centring", "mult", "crystal_system", "n_axes", "max_m", "zero", "status")


def tolerances(num_atoms, lattices, symprec=SYMPREC):
    """symprec / (V_b / n_b)^(1/3) per crystal as float64 numpy, V_b in float64 from the float32 cell (rows of the prepared set's units:
    unit volume per atom).  On the host, so that the device and the restatement read the same number; 1 where the cell has no volume (the
    prepare status flags such a crystal)."""
    L = np.asarray(lattices, np.float32).reshape(-1, 9).astype(np.float64)
    na = np.asarray(num_atoms, np.int64)
    out = np.ones(len(L))
    for b in range(len(L)):
        l = [float(x) for x in L[b]]
        v = abs((l[0] * (l[4] * l[8] - l[5] * l[7]) - l[1] * (l[3] * l[8] - l[5] * l[6])) + l[2] * (l[3] * l[7] - l[4] * l[6]))
        if na[b] >= 1 and math.isfinite(v) and v > 0.0:
            out[b] = float(symprec) / (v / int(na[b])) ** (1.0 / 3.0)
    return out


class SymmetryResult:
    """The arrays of mi_sym_find on the device (info [B, 8], rot_hist [B, 10], rot [B, 192, 9], trans [B, 192, 3], dev [B, 192], ptrans
    [B, 64, 3]) and, read once, the named columns of info as numpy."""

    def __init__(self, info, rot_hist, rot, trans, dev, ptrans, tol):
        self.info, self.rot_hist, self.rot, self.trans, self.dev, self.ptrans, self.tol = info, rot_hist, rot, trans, dev, ptrans, tol
        self._host = None

    def __len__(self):
        return len(self.info)

    def host(self):
        if self._host is None:
            self._host = self.info.cpu().numpy()
        return self._host

    def __getattr__(self, name):
        if name in INFO:
            return self.host()[:, INFO.index(name)].copy()
        raise AttributeError(name)

    @property
    def point_group(self):
        """Hermann-Mauguin symbols; "" where the classes are those of no point group or the crystal was not analysed."""
        return [POINT_GROUPS[i] for i in self.host()[:, 4]]

    @property
    def crystal_system_name(self):
        return [CRYSTAL_SYSTEMS[i] for i in self.host()[:, 5]]

    def operations(self, i):
        """(W [k, 3, 3] int, t [k, 3], dev [k]) of crystal i in the basis of its reduced cell: f' = wrap(f W^-1 + t); k = min(n_ops, 192)."""
        k = min(int(self.host()[i, 0]), _lib.SYM_MAX_OPS)
        return self.rot[i, :k].reshape(k, 3, 3).cpu().numpy(), self.trans[i, :k].cpu().numpy(), self.dev[i, :k].cpu().numpy()


def find_symmetry_prepared(prepared, tol, angle_tol=ANGLE_TOL, fill=None):
    """mi_sym_find on a prepared set (matching.Prepared) and its tolerances (float64 [B], the prepared set's units).  `fill` builds the
    output tensors (tests poison them)."""
    lib = _lib.load()
    dev = prepared.lat.device
    B = prepared.B
    tol = torch.as_tensor(np.asarray(tol, np.float64) if not torch.is_tensor(tol) else tol, dtype=torch.float64, device=dev).contiguous()
    z = (lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)) if fill is None else fill
    res = SymmetryResult(z((B, _lib.SYM_INFO), torch.int32), z((B, _lib.SYM_CLASSES), torch.int32), z((B, _lib.SYM_MAX_OPS, 9), torch.int32),
                         z((B, _lib.SYM_MAX_OPS, 3), torch.float64), z((B, _lib.SYM_MAX_OPS), torch.float64), z((B, _lib.SYM_MAX_TRANS, 3), torch.float64), tol)
    if B:
        if tol.numel() != B:
            raise ValueError(f"find_symmetry_prepared: {tol.numel()} tolerances for {B} crystals")
        st = prepared.struct()
        out = _lib.SymOut(*(t.data_ptr() for t in (res.info, res.rot_hist, res.rot, res.trans, res.dev, res.ptrans)))
        _lib.check(lib.mi_sym_find(C.byref(st), tol.data_ptr(), math.cos(math.radians(float(angle_tol))), C.byref(out), torch.cuda.current_stream().cuda_stream),
                   "mi_sym_find")
    return res


class Primitive:
    """The arrays of mi_sym_primitive on the device: offsets [B + 1], types, frac [N, 3] float32 (the first offsets[B] rows), lat [B, 9]
    float32, count, status [B], det [B]."""

    def __init__(self, offsets, types, frac, lat, count, status, det):
        self.offsets, self.types, self.frac, self.lat, self.count, self.status, self.det = offsets, types, frac, lat, count, status, det


def primitive_arrays(prepared, types, frac, lat, sym, fill=None):
    """mi_sym_primitive on device tensors: the prepared set, the arrays it was prepared from and the SymmetryResult of it."""
    lib = _lib.load()
    dev = prepared.lat.device
    B, N = prepared.B, prepared.N
    types, frac, lat = types.to(torch.int32).contiguous(), frac.to(torch.float32).contiguous(), lat.to(torch.float32).reshape(-1, 9).contiguous()
    z = (lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)) if fill is None else fill
    M = max(N, 1)
    ws_types, ws_frac = torch.zeros(M, dtype=torch.int32, device=dev), torch.zeros((M, 3), dtype=torch.float32, device=dev)
    out = Primitive(z((B + 1,), torch.int32), z((M,), torch.int32), z((M, 3), torch.float32), z((B, 9), torch.float32), z((B,), torch.int32),
                    z((B,), torch.int32), z((B,), torch.float64))
    if B:
        p = lambda t: t.data_ptr()
        args = _lib.SymPrimArgs(prepared.struct(), p(types), p(frac), p(lat), p(sym.info), p(sym.ptrans), p(ws_types), p(ws_frac), p(out.count), p(out.status),
                                p(out.det), p(out.offsets), p(out.types), p(out.frac), p(out.lat))
        _lib.check(lib.mi_sym_primitive(C.byref(args), torch.cuda.current_stream().cuda_stream), "mi_sym_primitive")
    return out


def _upload(records, device, symprec):
    na, types, frac, lat = record_arrays(records)
    offsets = torch.cat([torch.zeros(1, dtype=torch.long), na.cumsum(0)]).to(torch.int32)
    dev = torch.device(device)
    return na, offsets.to(dev), types.to(dev), frac.to(dev), lat.reshape(-1, 9).to(dev), tolerances(na.numpy(), lat.numpy(), symprec)


def find_symmetry(records, symprec=SYMPREC, angle_tol=ANGLE_TOL, device="cuda"):
    """The SymmetryResult of host records (SimpleStructure / CrystalData-like): one upload, two launches.  Never drops or reorders; a
    record the prepare guard flags has status NOT_PREPARED and zero counts."""
    na, offsets, types, frac, lat, tol = _upload(records, device, symprec)
    prepared = matching.prepare_arrays(offsets, types, frac, lat)
    return find_symmetry_prepared(prepared, tol, angle_tol)


def reduce_arrays(offsets, types, frac, lat, tol, angle_tol=ANGLE_TOL):
    """prepare -> mi_sym_find -> mi_sym_primitive on device tensors: (Primitive, SymmetryResult)."""
    prepared = matching.prepare_arrays(offsets, types, frac, lat)
    sym = find_symmetry_prepared(prepared, tol, angle_tol)
    return primitive_arrays(prepared, types, frac, lat, sym), sym


def primitive_records(records, symprec=SYMPREC, angle_tol=ANGLE_TOL, device="cuda"):
    """(records, n_trans): every record in its primitive cell as a SimpleStructure (a record with one pure translation, or whose analysis
    is not OK, keeps its cell and coordinates), and the number of pure translations found per record."""
    from .data import SimpleStructure
    if len(records) == 0:
        return [], np.zeros(0, np.int64)
    na, offsets, types, frac, lat, tol = _upload(records, device, symprec)
    prim, sym = reduce_arrays(offsets, types, frac, lat, tol, angle_tol)
    off, z, f, L = prim.offsets.cpu().numpy(), prim.types.cpu().numpy(), prim.frac.cpu().numpy(), prim.lat.cpu().numpy().reshape(-1, 3, 3).astype(np.float64)
    out = []
    for b in range(len(records)):
        lengths = np.linalg.norm(L[b], axis=1)
        cos = [float(np.dot(L[b][i], L[b][j]) / (lengths[i] * lengths[j])) for i, j in ((1, 2), (0, 2), (0, 1))]
        angles = [math.degrees(math.acos(max(-1.0, min(1.0, c)))) for c in cos]
        out.append(SimpleStructure([float(x) for x in lengths], angles, [int(v) for v in z[off[b]:off[b + 1]]], f[off[b]:off[b + 1]].astype(np.float64)))
    return out, sym.n_trans.astype(np.int64)


# ---- the conventional cell ----------------------------------------------------------------------------------------------------------
class Conventional:
    """The arrays of mi_sym_conventional on the device: info [B, 8], M [B, 9], cvec [B, 4, 3], count [B], offsets [B + 1], types [4 N], frac
    [4 N, 3] float32 (the first offsets[B] rows), lat [B, 9] float32."""

    def __init__(self, info, M, cvec, count, offsets, types, frac, lat):
        self.info, self.M, self.cvec, self.count, self.offsets, self.types, self.frac, self.lat = info, M, cvec, count, offsets, types, frac, lat


def conventional_prepared(prepared, types, frac, lat, sym, fill=None):
    """mi_sym_conventional on device tensors: the prepared set of the primitive crystals, the arrays it was prepared from and the
    SymmetryResult of it.  `fill` builds the output tensors (tests poison them)."""
    lib = _lib.load()
    dev = prepared.lat.device
    B, N = prepared.B, prepared.N
    types, frac, lat = types.to(torch.int32).contiguous(), frac.to(torch.float32).contiguous(), lat.to(torch.float32).reshape(-1, 9).contiguous()
    z = (lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)) if fill is None else fill
    rows = max(4 * N, 1)
    ws_adj = torch.zeros((B, 9), dtype=torch.int32, device=dev)
    out = Conventional(z((B, _lib.SYM_CONV_INFO), torch.int32), z((B, 9), torch.int32), z((B, _lib.SYM_CONV_MAX_MULT, 3), torch.int32), z((B,), torch.int32),
                       z((B + 1,), torch.int32), z((rows,), torch.int32), z((rows, 3), torch.float32), z((B, 9), torch.float32))
    if B:
        p = lambda t: t.data_ptr()
        args = _lib.SymConvArgs(prepared.struct(), p(types), p(frac), p(lat), p(sym.info), p(sym.rot), p(ws_adj), p(out.info), p(out.M), p(out.cvec), p(out.count),
                                p(out.offsets), p(out.types), p(out.frac), p(out.lat))
        _lib.check(lib.mi_sym_conventional(C.byref(args), torch.cuda.current_stream().cuda_stream), "mi_sym_conventional")
    return out


def conventional_arrays(offsets, types, frac, lat, tol, angle_tol=ANGLE_TOL):
    """prepare -> mi_sym_find -> mi_sym_primitive -> prepare -> mi_sym_find -> mi_sym_conventional on device tensors, nothing read back
    between them: (Conventional, SymmetryResult of the primitive crystals).  The second analysis runs with the first one's tolerances: they
    are in the prepared set's units (unit volume per atom), which the primitive cell keeps."""
    prim, _ = reduce_arrays(offsets, types, frac, lat, tol, angle_tol)
    prepared = matching.prepare_arrays(prim.offsets, prim.types, prim.frac, prim.lat)
    sym = find_symmetry_prepared(prepared, tol, angle_tol)
    return conventional_prepared(prepared, prim.types, prim.frac, prim.lat, sym), sym


class ConventionalResult:
    """Per record, as numpy: bravais (Pearson-style strings, "" where there is no conventional cell), bravais_index (1 .. 14, 0), centring
    ("P", "A", "B", "C", "I", "F", "R", ""), mult, crystal_system, M [B, 3, 3] (the conventional vectors in the reduced primitive basis),
    status (the find status of the primitive crystal, with SYM_CONV_FAIL = 512 where the record came back as it was) and cell_parameters
    [B, 6] (a, b, c, alpha, beta, gamma of the returned records)."""

    def __init__(self, info, M, cell_parameters):
        self.info = info
        self.bravais_index, self.mult, self.crystal_system, self.status = (info[:, k].copy() for k in (0, 2, 3, 7))
        self.bravais = [BRAVAIS[i] for i in info[:, 0]]
        self.centring = [CENTRINGS[i] for i in info[:, 1]]
        self.M, self.cell_parameters = M, cell_parameters

    def __len__(self):
        return len(self.info)


def _parameters(L):
    lengths = np.linalg.norm(L, axis=1)
    cos = [float(np.dot(L[i], L[j]) / (lengths[i] * lengths[j])) for i, j in ((1, 2), (0, 2), (0, 1))]
    return [float(x) for x in lengths], [math.degrees(math.acos(max(-1.0, min(1.0, c)))) for c in cos]


def conventional_records(records, symprec=SYMPREC, angle_tol=ANGLE_TOL, device="cuda"):
    """(records, ConventionalResult): every record in its conventional cell as a SimpleStructure.  Never drops or reorders; a record
    without a conventional cell (any status but OK) comes back as it was."""
    from .data import SimpleStructure
    if len(records) == 0:
        return [], ConventionalResult(np.zeros((0, _lib.SYM_CONV_INFO), np.int32), np.zeros((0, 3, 3), np.int32), np.zeros((0, 6)))
    na, offsets, types, frac, lat, tol = _upload(records, device, symprec)
    conv, _ = conventional_arrays(offsets, types, frac, lat, tol, angle_tol)
    info, M = conv.info.cpu().numpy(), conv.M.cpu().numpy().reshape(-1, 3, 3)
    off, z, f, L = conv.offsets.cpu().numpy(), conv.types.cpu().numpy(), conv.frac.cpu().numpy(), conv.lat.cpu().numpy().reshape(-1, 3, 3).astype(np.float64)
    out, params = [], np.full((len(records), 6), np.nan)
    for b, rec in enumerate(records):
        if info[b, 7] != _lib.SYM_OK or info[b, 0] == 0:
            out.append(rec)
            try:
                params[b] = list(np.asarray(rec.lengths, np.float64).reshape(-1)) + list(np.asarray(rec.angles, np.float64).reshape(-1))
            except Exception:
                pass
            continue
        lengths, angles = _parameters(L[b])
        params[b] = lengths + angles
        out.append(SimpleStructure(lengths, angles, [int(v) for v in z[off[b]:off[b + 1]]], f[off[b]:off[b + 1]].astype(np.float64)))
    return out, ConventionalResult(info, M, params)


# ---- the refined structure ----------------------------------------------------------------------------------------------------------
REFINE_INFO = ("n_orbits", "n_ops", "zero2", "zero3", "zero4", "zero5", "zero6", "status")
REFINE_STAT = ("max_move", "rms_move", "cell_change", "max_residual")
REFINE_CELLS = ("given", "primitive", "conventional")


class Refined:
    """The arrays of mi_sym_refine on the device, with the arrays it refined: offsets [B + 1], types [rows] (the first offsets[B] rows are
    atoms), frac [rows, 3] and lat [B, 9] float32 (refined), orbit, mult, site_order [rows] (orbit: the lowest equivalent atom, an index
    inside its crystal), trans_ref [B, 192, 3], info [B, 8] (n_orbits, n_ops, .., status), stat [B, 4] float64 (max move, rms move, cell
    change, max residual in the prepared set's units) and tol [B], the tolerances the analysis ran with."""

    def __init__(self, offsets, types, frac, lat, orbit, mult, site_order, trans_ref, info, stat, tol=None):
        self.offsets, self.types, self.frac, self.lat, self.orbit, self.mult, self.site_order = offsets, types, frac, lat, orbit, mult, site_order
        self.trans_ref, self.info, self.stat, self.tol = trans_ref, info, stat, tol


def refine_prepared(prepared, types, frac, lat, sym, fill=None):
    """mi_sym_refine on device tensors: the prepared set, the arrays it was prepared from and the SymmetryResult of it.  `fill` builds the
    output tensors (tests poison them)."""
    lib = _lib.load()
    dev = prepared.lat.device
    B, N = prepared.B, prepared.N
    types, frac, lat = types.to(torch.int32).contiguous(), frac.to(torch.float32).contiguous(), lat.to(torch.float32).reshape(-1, 9).contiguous()
    z = (lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)) if fill is None else fill
    M = max(N, 1)
    out = Refined(prepared.offsets, types, z((M, 3), torch.float32), z((B, 9), torch.float32), z((M,), torch.int32), z((M,), torch.int32), z((M,), torch.int32),
                  z((B, _lib.SYM_MAX_OPS, 3), torch.float64), z((B, _lib.SYM_REFINE_INFO), torch.int32), z((B, _lib.SYM_REFINE_STAT), torch.float64), sym.tol)
    if B:
        p = lambda t: t.data_ptr()
        args = _lib.SymRefineArgs(prepared.struct(), p(types), p(frac), p(lat), p(sym.info), p(sym.rot), p(sym.trans), p(out.frac), p(out.lat), p(out.orbit),
                                  p(out.mult), p(out.site_order), p(out.trans_ref), p(out.info), p(out.stat))
        _lib.check(lib.mi_sym_refine(C.byref(args), torch.cuda.current_stream().cuda_stream), "mi_sym_refine")
    return out


def _refine_stage(offsets, types, frac, lat, tol, angle_tol, earlier=None):
    """prepare -> find -> refine of one stage's arrays.  A crystal the prepare guard rejects (a conventional cell of more than 64 atoms) has
    nothing written by the entry: its rows come back as this stage received them, every atom an orbit of its own.  `earlier`: the fail bits
    of the stages before ([B] int32), joined to the status."""
    types, frac, lat = types.to(torch.int32).contiguous(), frac.to(torch.float32).contiguous(), lat.to(torch.float32).reshape(-1, 9).contiguous()
    prepared = matching.prepare_arrays(offsets, types, frac, lat)
    sym = find_symmetry_prepared(prepared, tol, angle_tol)
    out = refine_prepared(prepared, types, frac, lat, sym)
    B, rows = prepared.B, out.frac.shape[0]
    if B:
        off = offsets.to(torch.int64)
        skipped = (out.info[:, -1] & _lib.SYM_NOT_PREPARED) != 0                                                 # [B]
        atom = torch.arange(rows, device=off.device)
        owner = torch.searchsorted(off[1:].contiguous(), atom, right=True).clamp_(max=B - 1)                  # the crystal of a row
        mine = skipped[owner]
        local, one = (atom - off[owner]).to(torch.int32), torch.ones_like(out.mult)
        if prepared.N:
            out.frac = torch.where(mine[:, None], frac[:rows], out.frac)
            out.orbit, out.mult, out.site_order = torch.where(mine, local, out.orbit), torch.where(mine, one, out.mult), torch.where(mine, one, out.site_order)
        out.lat = torch.where(skipped[:, None], lat, out.lat)
        if earlier is not None:
            out.info[:, -1] |= earlier.to(torch.int32)
    return out


def refine_arrays(offsets, types, frac, lat, tol, angle_tol=ANGLE_TOL, cell="given"):
    """The refined crystals on device tensors, nothing read back in between: a Refined.  cell="given": prepare -> mi_sym_find ->
    mi_sym_refine.  cell="primitive": reduce_arrays first, then the same on its output.  cell="conventional": conventional_arrays first,
    then the same.  The later analyses run with the caller's tolerances: they are in the prepared set's units (unit volume per atom), which
    both changes of cell keep.  A crystal a later stage cannot take comes back as the stage before produced it, with SYM_REFINE_FAIL; a
    crystal an earlier stage left as it was (SYM_PRIM_FAIL, SYM_CONV_FAIL) is refined in the cell it has and carries that bit."""
    if cell not in REFINE_CELLS:
        raise ValueError(f"refine_arrays: cell {cell!r} is none of {REFINE_CELLS}")
    if cell == "given":
        return _refine_stage(offsets, types, frac, lat, tol, angle_tol)
    if cell == "primitive":
        prim, _ = reduce_arrays(offsets, types, frac, lat, tol, angle_tol)
        return _refine_stage(prim.offsets, prim.types, prim.frac, prim.lat, tol, angle_tol, prim.status & _lib.SYM_PRIM_FAIL)
    conv, _ = conventional_arrays(offsets, types, frac, lat, tol, angle_tol)
    return _refine_stage(conv.offsets, conv.types, conv.frac, conv.lat, tol, angle_tol, conv.info[:, -1] & _lib.SYM_CONV_FAIL)


class RefineResult:
    """Per record, as numpy, from one read: status (the find status of the cell refined, with SYM_REFINE_FAIL = 1024 where the record came
    back as it was), n_ops, n_orbits (symmetry-inequivalent sites), max_move, rms_move and max_residual in A (the prepared set's units
    times (V / n)^(1/3) of the record), cell_change (max |Gbar - G| / max |G|), cell_parameters [B, 6] of the returned records, and per
    record i orbits(i), multiplicity(i), site_symmetry_order(i) in the atom order of the returned record."""

    def __init__(self, info, stat, scale, offsets, orbit, mult, site_order, cell_parameters):
        self.info, self.offsets, self._orbit, self._mult, self._site = info, offsets, orbit, mult, site_order
        self.status, self.n_orbits, self.n_ops = info[:, 7].copy(), info[:, 0].copy(), info[:, 1].copy()
        self.max_move, self.rms_move, self.max_residual = stat[:, 0] * scale, stat[:, 1] * scale, stat[:, 3] * scale
        self.cell_change, self.cell_parameters = stat[:, 2].copy(), cell_parameters

    def __len__(self):
        return len(self.info)

    def _rows(self, arr, i):
        return arr[int(self.offsets[i]):int(self.offsets[i + 1])].copy()

    def orbits(self, i):
        """Per atom of record i the lowest equivalent atom (an index into the record)."""
        return self._rows(self._orbit, i)

    def multiplicity(self, i):
        return self._rows(self._mult, i)

    def site_symmetry_order(self, i):
        return self._rows(self._site, i)


def refined_records(records, symprec=SYMPREC, angle_tol=ANGLE_TOL, device="cuda", cell="given"):
    """(records, RefineResult): every record with its coordinates and its cell projected onto the group found at symprec, as a
    SimpleStructure in the cell asked for ("given", "primitive", "conventional").  Never drops or reorders; a record whose status is not OK
    is returned as the same object, with one orbit per atom."""
    from .data import SimpleStructure
    if cell not in REFINE_CELLS:
        raise ValueError(f"refined_records: cell {cell!r} is none of {REFINE_CELLS}")
    if len(records) == 0:
        e = np.zeros(0, np.int32)
        return [], RefineResult(np.zeros((0, _lib.SYM_REFINE_INFO), np.int32), np.zeros((0, _lib.SYM_REFINE_STAT)), np.zeros(0), np.zeros(1, np.int64), e, e, e,
                                np.zeros((0, 6)))
    na, offsets, types, frac, lat, tol = _upload(records, device, symprec)
    ref = refine_arrays(offsets, types, frac, lat, tol, angle_tol, cell)
    info, stat, off = ref.info.cpu().numpy(), ref.stat.cpu().numpy(), ref.offsets.cpu().numpy().astype(np.int64)
    z, f, L = ref.types.cpu().numpy(), ref.frac.cpu().numpy(), ref.lat.cpu().numpy().reshape(-1, 3, 3).astype(np.float64)
    orbit, mult, site = (t.cpu().numpy().copy() for t in (ref.orbit, ref.mult, ref.site_order))
    scale = float(symprec) / np.asarray(tol, np.float64)   # (V / n)^(1/3) of every record: the changes of cell keep V / n
    out, params, out_off = [], np.full((len(records), 6), np.nan), [0]
    o2, m2, s2 = [], [], []
    for b, rec in enumerate(records):
        lo, hi = int(off[b]), int(off[b + 1])
        if info[b, 7] != _lib.SYM_OK:
            out.append(rec)
            n = int(na[b])
            o2.append(np.arange(n, dtype=np.int32)), m2.append(np.ones(n, np.int32)), s2.append(np.ones(n, np.int32))
            info[b, 0] = n
            stat[b] = 0.0
            try:
                params[b] = list(np.asarray(rec.lengths, np.float64).reshape(-1)) + list(np.asarray(rec.angles, np.float64).reshape(-1))
            except Exception:
                pass
        else:
            lengths, angles = _parameters(L[b])
            params[b] = lengths + angles
            out.append(SimpleStructure(lengths, angles, [int(v) for v in z[lo:hi]], f[lo:hi].astype(np.float64)))
            o2.append(orbit[lo:hi]), m2.append(mult[lo:hi]), s2.append(site[lo:hi])
        out_off.append(out_off[-1] + len(o2[-1]))
    return out, RefineResult(info, stat, scale, np.asarray(out_off, np.int64), np.concatenate(o2), np.concatenate(m2), np.concatenate(s2), params)


def symmetry_primitive_records(records, symprec=SYMPREC, angle_tol=ANGLE_TOL, device="cuda"):
    """refined_records(..., cell="primitive"): the refined structure in its primitive cell, the place of the reference's
    get_symmetry_primitive (SpacegroupAnalyzer(symprec=0.1).get_refined_structure().get_primitive_structure()).  The choice of cell is this
    build's own (the first basis triple of the translation lattice); pymatgen's choice is [UPSTREAM-UNVERIFIED] (it is absent
    here) and is not claimed to be reproduced."""
    return refined_records(records, symprec, angle_tol, device, cell="primitive")
