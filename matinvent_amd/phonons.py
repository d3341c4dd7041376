"""Phonons on a q-mesh of a learned energy from displacements of the home cell of a supercell: force constants, dynamical matrices at any
q, dynamical stability over the zone, the harmonic heat capacity per primitive cell and dispersion curves, on the device
(include/matinvent_hip_phonon.h).

The reference's phonon reward (rewards/calculators/fairchem/phonon.py) builds a supercell with min_lengths = 10, displaces the atoms of one
cell only and takes the heat capacity from a q-mesh over the Brillouin zone.  vibrations.Vibrations(supercell=reps) reaches the
commensurate q-points by displacing every atom of every image and diagonalising one matrix of order 3 n N - 3.  Here a record of n atoms is
replicated (structure.make_supercell: image 0 first, its atoms in their own order), the 6 n copies that displace a HOME atom go through
mi_vib_run_chunk as they stand -- N times fewer gradient evaluations -- and behind the last chunk: mi_phonon_fc (central differences, the
index symmetry, the acoustic sum rule, the shortest-image table), then per chunk of (crystal, q) items mi_phonon_dynmat (D(q) as a real
symmetric matrix of order 6 n) and mi_sym_eigvals, then mi_phonon_thermo (frequencies in THz, weighted counts, c_v(T), the zero-point
energy, the lowest frequency and its q).  The device evaluates no transcendental function in front of the eigenvalues: the phases
e^{2 pi i q_d r_d} come from phase_table below, one numpy function that the tests' restatement also calls.  Everything is enqueued on the
current stream and nothing is read before the caller reads.

Departures and limits, stated: the supercell is DIAGONAL (the reference's transformation may be non-diagonal); the mesh is reduced by
q <-> -q only; the shortest-image search covers the 27 neighbouring supercells; mesh, tie_tol, delta and nu_cut ship UNTUNED, and no weight
of this repository is trained: nothing about the quality of a frequency or a heat capacity is claimed."""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import energy_analysis as EA
from . import vibrations as VB
from .energy_analysis import _at, release_handles   # noqa: F401  (release_handles follows the read of a state)
from .vibrations import KB_J_MOL, STATUS   # noqa: F401

# the (crystal, q) matrices of one mi_phonon_dynmat / mi_sym_eigvals launch pair stay under this many bytes (the eigen-solver's work copies
# included); an analysis of more items runs in several launch pairs on one buffer.  256 MiB: 1820 matrices of order 120 in the LDS path.
WORKSPACE_CAP = 256 << 20

MeshPoints = namedtuple("MeshPoints", "q weights k mesh")


def mesh_points(mesh):
    """The Gamma-centred grid k / mesh, k_d = 0 .. mesh_d - 1, reduced by q <-> -q (D(-q) = conj D(q)): of each pair the lexicographically
    smaller k is kept with weight 2, a point that is its own partner with weight 1.  MeshPoints(q [Q][3] float64, weights [Q] int32,
    k [Q][3] int64, mesh); the weights sum to mesh_a mesh_b mesh_c."""
    m = tuple(int(v) for v in mesh)
    if len(m) != 3 or min(m) < 1:
        raise ValueError(f"mesh_points: mesh = {mesh}: three integers >= 1")
    ks, ws = [], []
    for a in range(m[0]):
        for b in range(m[1]):
            for c in range(m[2]):
                k, neg = (a, b, c), ((-a) % m[0], (-b) % m[1], (-c) % m[2])
                if k <= neg:
                    ks.append(k)
                    ws.append(1 if k == neg else 2)
    k = np.asarray(ks, dtype=np.int64)
    return MeshPoints(k / np.asarray(m, dtype=np.float64), np.asarray(ws, dtype=np.int32), k, m)


def _unit_phase(x):
    """(cos, sin) of 2 pi x for x reduced to [-1/2, 1/2]: the multiples of a quarter turn exactly, and conjugate under x -> -x bit for bit."""
    sign, ax = (-1.0 if x < 0 else 1.0), abs(x)
    if ax == 0.0:
        return 1.0, 0.0
    if ax == 0.5:
        return -1.0, 0.0
    if ax == 0.25:
        return 0.0, sign
    return float(np.cos(2.0 * np.pi * ax)), sign * float(np.sin(2.0 * np.pi * ax))


def phase_table(qpoints, reps):
    """The host table of mi_phonon_dynmat, float64 [Q][6 (a + b + c)]: per q the axes in order, per axis the 3 reps_d entries (re, im) of
    e^{2 pi i q_d r_d}, r_d = -reps_d .. 2 reps_d - 1.  qpoints: a MeshPoints (q_d = k / m: the argument is reduced in integers first,
    (k r_d mod m) / m, so a commensurate phase is the same number whichever r_d reaches it) or an array [Q][3] of fractional reciprocal
    coordinates of the primitive cell."""
    reps = tuple(int(r) for r in reps)
    exact = isinstance(qpoints, MeshPoints)
    pts = qpoints.k if exact else np.asarray(qpoints, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((len(pts), 6 * sum(reps)), dtype=np.float64)
    for iq, pt in enumerate(pts):
        at = 0
        for d in range(3):
            for r in range(-reps[d], 2 * reps[d]):
                if exact:
                    m = int(qpoints.mesh[d])
                    num = (int(pt[d]) * r) % m
                    num = num - m if 2 * num > m else num
                    x = num / m
                else:
                    arg = float(pt[d]) * r
                    x = arg - np.rint(arg)
                out[iq, at], out[iq, at + 1] = _unit_phase(x)
                at += 2
    return out


def auto_reps(lattice, min_length):
    """reps_d = ceil(min_length / h_d), h_d = V / |a_e x a_f|: the spacing of the lattice planes that axis d crosses (rows are cell vectors)."""
    L = np.asarray(lattice, dtype=np.float64).reshape(3, 3)
    V = abs(np.linalg.det(L))
    out = []
    for d in range(3):
        area = np.linalg.norm(np.cross(L[(d + 1) % 3], L[(d + 2) % 3]))
        h = V / area if area > 0 else 0.0
        if not (np.isfinite(h) and h > 0):
            return None
        out.append(max(1, int(np.ceil(float(min_length) / h - 1e-12))))
    return tuple(out)


class Phonons(VB.HarmonicAnalysis):
    """What an analysis needs: predictor, task, delta, per_atom, temperatures, nu_cut, batch_size, det_min as vibrations.Vibrations';
    supercell: (a, b, c) or "auto" (auto_reps with min_length, per record); mesh: the Gamma-centred q-mesh of analyze_records; tie_tol: the
    distance (Angstrom) within which two images of a pair count as equally near (1e-5: phonopy's symprec from memory, unverified);
    workspace_cap: bytes of (crystal, q) matrices per launch pair."""

    def __init__(self, predictor, task, supercell=(2, 2, 2), min_length=10.0, mesh=(4, 4, 4), delta=0.01, per_atom=True, temperatures=(300.0,), nu_cut=0.05,
                 batch_size=256, tie_tol=1e-5, det_min=1e-3, workspace_cap=WORKSPACE_CAP):
        super().__init__(predictor, task, delta, per_atom, temperatures, nu_cut, batch_size, det_min)
        if isinstance(supercell, str):
            if supercell != "auto":
                raise ValueError(f"Phonons: supercell = {supercell!r}: three integers >= 1 or \"auto\"")
            sc = "auto"
        else:
            sc = tuple(int(r) for r in supercell)
            if len(sc) != 3 or min(sc) < 1:
                raise ValueError(f"Phonons: supercell = {supercell}: three integers >= 1 or \"auto\"")
        if not (np.isfinite(float(min_length)) and float(min_length) > 0):
            raise ValueError(f"Phonons: min_length = {min_length}: must be finite and positive")
        if not (np.isfinite(float(tie_tol)) and float(tie_tol) >= 0):
            raise ValueError(f"Phonons: tie_tol = {tie_tol}: must be finite and >= 0")
        if int(workspace_cap) < 1:
            raise ValueError(f"Phonons: workspace_cap = {workspace_cap}: must be >= 1")
        self.mesh = mesh_points(mesh).mesh
        self.supercell, self.min_length, self.tie_tol, self.workspace_cap = sc, float(min_length), float(tie_tol), int(workspace_cap)

    def reps_for(self, lattice):
        return self.supercell if self.supercell != "auto" else auto_reps(lattice, self.min_length)


def chunk_plan(prim_atoms, batch_size):
    """The displaced copies of the HOME atoms of supercells whose primitive cells have prim_atoms atoms: (source crystal, c = 6 i + 2 d + s),
    i < n, in order: a list of (src [k] int32, copy [k] int32) -- vibrations.chunk_plan on the primitive counts, since make_supercell
    puts the home cell's atoms first.  The ceil(total / batch_size) chunks are BALANCED (each ceil(total / chunks) copies, the last one
    what is left) rather than filled to batch_size: a handle is made per distinct chunk shape and costs more than a gradient evaluation
    (DESIGN 51), and equal crystals in balanced chunks share one."""
    total, bs = 6 * int(np.sum(np.asarray(prim_atoms, dtype=np.int64))), int(batch_size)
    if total == 0:
        return []
    chunks = -(-total // bs)
    return VB.chunk_plan(prim_atoms, -(-total // chunks))


def _reps_array(reps):
    return (C.c_int * 3)(*[int(r) for r in reps])


def ws_layout(num_atoms, reps):
    """(bytes, o [B + 1] doubles) of mi_phonon_workspace; its refusals raise _lib.MIError by name."""
    na = (C.c_int * max(len(num_atoms), 1))(*[int(n) for n in num_atoms])
    off = (C.c_int64 * (len(num_atoms) + 1))()
    nbytes = _lib.load().mi_phonon_workspace(na, _reps_array(reps), len(num_atoms), off)
    if nbytes < 0:
        _lib.check(int(nbytes), "mi_phonon_workspace")
    return int(nbytes), np.asarray(list(off), dtype=np.int64)


def item_chunks(sizes, cap_bytes, need_work):
    """Cut the item list [0, T) into consecutive ranges whose matrices (and work copies) stay under cap_bytes; a range holds one item at
    least.  Returns [(start, stop)] and the items' matrix offsets (doubles) inside their range's buffer."""
    per = 16 if need_work else 8
    cuts, off, start, used = [], np.zeros(len(sizes), np.int64), 0, 0
    for t, M in enumerate(sizes):
        b = per * int(M) * int(M)
        if t > start and used + b > cap_bytes:
            cuts.append((start, t))
            start, used = t, 0
        off[t] = used // per
        used += b
    if len(sizes) > start:
        cuts.append((start, len(sizes)))
    return cuts, off


def source_arrays(p, state, num_atoms, masses, reps, table, weights, no_lds=0):
    """The device arrays of an analysis of the supercell state (frac_coords [N][3], lattices [B][3][3], atom_types [N][100] float rows) of
    supercells of num_atoms atoms with masses [N] (amu), each the reps-fold replica of its primitive cell, at the Q points of `table`
    (phase_table's) with integer weights: the state as float32, the offsets, the workspace, the item list and every output."""
    dev = p.predictor.device
    na = [int(n) for n in num_atoms]
    reps = tuple(int(r) for r in reps)
    Nimg = reps[0] * reps[1] * reps[2]
    nbytes, o = ws_layout(na, reps)   # (refuses what does not divide)
    prim = [n // Nimg for n in na]
    B, N, Q = len(na), int(sum(na)), int(len(weights))
    table = np.ascontiguousarray(table, dtype=np.float64)
    x, l, a = state
    f = lambda t: t.to(dev, torch.float32).contiguous()
    up = lambda arr, dt: torch.from_numpy(np.ascontiguousarray(arr)).to(dt).to(dev)
    e = lambda *s, dt=torch.float64: torch.empty(*s, device=dev, dtype=dt)
    n64 = np.asarray(na, dtype=np.int64)
    sizes = np.repeat(6 * np.asarray(prim, dtype=np.int64), Q)
    ev_off = np.concatenate([[0], np.cumsum(sizes)])
    need_work = bool(no_lds) or (sizes.size > 0 and int(sizes.max()) > _lib.EIG_LDS_MAX_M)
    cuts, mat_off = item_chunks(sizes, p.workspace_cap, need_work)
    mat_doubles = max([int((sizes[s:t] ** 2).sum()) for s, t in cuts] + [1])
    T, K = len(sizes), len(p.temperatures)
    return dict(frac=f(x), lat=f(l), types=f(a), na=na, prim=prim, reps=reps, B=B, N=N, Q=Q, T=T, node_off=up(np.concatenate([[0], np.cumsum(n64)]), torch.int32),
                mass=up(np.asarray(masses, dtype=np.float64), torch.float64), ws=e(max(nbytes // 8, 1)), ws_off=up(o[:-1], torch.int64), ws_off_host=o,
                table=up(table.reshape(-1), torch.float64), table_len=int(table.size), weight=up(np.asarray(weights, dtype=np.int32), torch.int32),
                item_crystal=up(np.repeat(np.arange(B, dtype=np.int32), Q), torch.int32), item_q=up(np.tile(np.arange(Q, dtype=np.int32), B), torch.int32),
                item_off=up(np.arange(B + 1, dtype=np.int32) * Q, torch.int32), sizes=up(sizes, torch.int32), mat_off=up(mat_off, torch.int64), cuts=cuts,
                need_work=need_work, mats=e(mat_doubles), work=e(mat_doubles) if need_work else None, ev_off=up(ev_off[:-1], torch.int64), ev_off_host=ev_off,
                evals=e(max(int(ev_off[-1]), 1)), lam=e(max(int(ev_off[-1]) // 2, 1)), freqs=e(max(int(ev_off[-1]) // 2, 1)), herm_item=e(max(T, 1)),
                sweeps=e(max(T, 1), dt=torch.int32), eig_status=e(max(T, 1), dt=torch.int32), asym=e(B), fc_status=e(B, dt=torch.int32), c_v=e(B, K), zpe=e(B),
                n_imag=e(B, dt=torch.int32), n_zero=e(B, dt=torch.int32), min_freq=e(B), min_q=e(B, dt=torch.int32), herm=e(B), pair_gap=e(B),
                sweeps_max=e(B, dt=torch.int32), status=e(B, dt=torch.int32), keep=[], handles=[])


def enqueue_gradients(p, src):
    """Every chunk's mi_vib_run_chunk on the current stream, the supercells as source and the home atoms' copies alone in the plan: the
    workspace's 6 n rows Gc of every crystal of `src` (vibrations.enqueue_gradients on this module's plan).  Returns the number of chunks."""
    return VB.enqueue_gradients(p, src, chunk_plan(src["prim"], p.batch_size))


def enqueue_fc(p, src):
    from .cspnet import _stream
    a = _lib.PhononFcArgs(_at(src["ws"]), _at(src["ws_off"]), _at(src["node_off"]), _at(src["mass"]), _at(src["frac"]), _at(src["lat"]), _at(src["asym"]),
                          _at(src["fc_status"]), p.delta, p.tie_tol, p.det_min, _reps_array(src["reps"]), src["B"], max(src["na"]) if src["na"] else 1)
    _lib.check(_lib.load().mi_phonon_fc(C.byref(a), _stream()), "mi_phonon_fc")


def _sub(t, start):
    """The device address of element `start` of a contiguous tensor."""
    return C.c_void_p(t.data_ptr() + int(start) * t.element_size())


def enqueue_dynmat(p, src, start, stop):
    """mi_phonon_dynmat on the items [start, stop) of one range of src["cuts"]."""
    from .cspnet import _stream
    a = _lib.PhononDynmatArgs(_at(src["ws"]), _at(src["ws_off"]), _at(src["node_off"]), _at(src["mass"]), _at(src["fc_status"]), _at(src["table"]),
                              _sub(src["item_crystal"], start), _sub(src["item_q"], start), _at(src["mats"]), _sub(src["mat_off"], start), _sub(src["sizes"], start),
                              _sub(src["herm_item"], start), src["table_len"], _reps_array(src["reps"]), src["B"], src["Q"], stop - start)
    _lib.check(_lib.load().mi_phonon_dynmat(C.byref(a), _stream()), "mi_phonon_dynmat")


def enqueue_eigvals(p, src, start, stop, no_lds=0):
    """mi_sym_eigvals, as it stands, on the matrices of the items [start, stop)."""
    from .cspnet import _stream
    a = _lib.SymEigArgs(_at(src["mats"]), _sub(src["mat_off"], start), _sub(src["sizes"], start), _at(src["work"]) if src["need_work"] else None, None, _at(src["evals"]),
                        _sub(src["ev_off"], start), _sub(src["sweeps"], start), _sub(src["eig_status"], start), stop - start, 6 * max(src["prim"]), int(no_lds))
    _lib.check(_lib.load().mi_sym_eigvals(C.byref(a), _stream()), "mi_sym_eigvals")


def enqueue_thermo(p, src):
    from .cspnet import _stream
    t = (C.c_double * 8)(*(list(p.temperatures) + [0.0] * (8 - len(p.temperatures))))
    a = _lib.PhononThermoArgs(*[_at(src[k]) for k in ("evals", "ev_off", "sizes", "eig_status", "sweeps", "herm_item", "fc_status", "item_off", "item_q", "weight",
                                                      "lam", "freqs", "c_v", "zpe", "n_imag", "n_zero", "min_freq", "min_q", "herm", "pair_gap", "sweeps_max", "status")],
                              t, p.nu_cut, src["B"], len(p.temperatures), src["Q"])
    _lib.check(_lib.load().mi_phonon_thermo(C.byref(a), _stream()), "mi_phonon_thermo")


def enqueue_spectrum(p, src, no_lds=0):
    """Everything behind the gradients: force constants, then per range of items the matrices and their eigenvalues, then the thermodynamics."""
    enqueue_fc(p, src)
    for start, stop in src["cuts"]:
        enqueue_dynmat(p, src, start, stop)
        enqueue_eigvals(p, src, start, stop, no_lds)
    enqueue_thermo(p, src)


def analyze_state(p, state, num_atoms, masses, reps, qpoints=None, weights=None, no_lds=0):
    """The whole analysis of a supercell state on the current stream, nothing read: the device arrays of source_arrays (freqs and lam
    [Q][3 n] per crystal at ev_off_host / 2; c_v [B][K], zpe, n_imag, n_zero, min_freq, min_q, asym, herm, pair_gap, sweeps_max, status [B]).
    qpoints: a MeshPoints (default: the analysis' mesh) or an array [Q][3] with weights (default 1).  Call release_handles(result) after
    the read."""
    qp = mesh_points(p.mesh) if qpoints is None else qpoints
    if weights is None:
        weights = qp.weights if isinstance(qp, MeshPoints) else np.ones(len(np.asarray(qp).reshape(-1, 3)), np.int32)
    src = source_arrays(p, state, num_atoms, masses, reps, phase_table(qp, reps), weights, no_lds)
    if src["B"] == 0 or src["Q"] == 0:
        return src
    with EA.releasing_on_error(src):
        enqueue_gradients(p, src)
        enqueue_spectrum(p, src, no_lds)
    return src


def _analyze(p, records, qpoints, weights):
    from .data import SimpleStructure
    from .predictor import _valid_fields
    from .structure import lattice_matrix, make_supercell
    dev = p.predictor.device
    records = list(records)
    n, K, Q = len(records), len(p.temperatures), len(weights)
    res = dict(frequencies=[np.zeros((Q, 0)) for _ in range(n)], n_imag=np.full(n, -1, np.int64), n_zero=np.full(n, -1, np.int64), c_v=np.full((n, K), np.nan),
               c_v_mol=np.full((n, K), np.nan), c_v_gram=np.full((n, K), np.nan), zpe=np.full(n, np.nan), min_freq=np.full(n, np.nan), min_q=np.full(n, -1, np.int64),
               asym=np.full(n, np.nan), herm=np.full(n, np.nan), pair_gap=np.full(n, np.nan), sweeps_max=np.full(n, -1, np.int64), status=np.full(n, -1, np.int64),
               reps=np.zeros((n, 3), np.int64), qpoints=np.asarray(qpoints.q if isinstance(qpoints, MeshPoints) else qpoints, dtype=np.float64).reshape(-1, 3),
               weights=np.asarray(weights, dtype=np.int64))
    fields, groups = [None] * n, {}
    for i, r in enumerate(records):
        f = _valid_fields(r)
        if f is None:
            continue
        z, x, le, an = f
        reps = p.reps_for(lattice_matrix(le, an))
        if reps is None:
            continue
        res["reps"][i] = reps
        N = reps[0] * reps[1] * reps[2]
        if z.size * N > _lib.VIB_MAX_ATOMS or z.size > _lib.PHONON_MAX_PRIM:
            continue   # refused, never silently shrunk: status -1
        try:
            big = make_supercell(SimpleStructure([float(v) for v in le], [float(v) for v in an], [int(v) for v in z], np.asarray(x, np.float64) % 1.0), reps)
        except (AttributeError, TypeError, ValueError, IndexError):
            continue
        fields[i] = _valid_fields(big)
        if fields[i] is not None:
            groups.setdefault(reps, []).append(i)

    def enqueue(reps, rows):
        na, state, mass = EA.pack_records(fields, rows, dev, masses=True)
        return rows, na, mass, analyze_state(p, state, na, mass, reps, qpoints, weights)

    def read(st):
        rows, na, mass, src = st
        cols = ("zpe", "min_freq", "asym", "herm", "pair_gap")
        ints = ("n_imag", "n_zero", "min_q", "sweeps_max", "status")
        small = torch.cat([src["c_v"]] + [src[k][:, None] for k in cols] + [src[k].to(torch.float64)[:, None] for k in ints], dim=1).cpu().numpy()
        freqs = src["freqs"].cpu().numpy()
        release_handles(src)
        off, eo = np.concatenate([[0], np.cumsum(na)]), src["ev_off_host"] // 2
        for k, i in enumerate(rows):
            prim = src["prim"][k]
            res["c_v"][i] = small[k, :K]
            res["c_v_mol"][i] = small[k, :K] * KB_J_MOL
            res["c_v_gram"][i] = small[k, :K] * KB_J_MOL / mass[off[k]:off[k] + prim].sum()
            for j, c in enumerate(cols):
                res[c][i] = small[k, K + j]
            for j, c in enumerate(ints):
                res[c][i] = int(small[k, K + len(cols) + j])
            res["frequencies"][i] = freqs[eo[k * Q]:eo[(k + 1) * Q]].reshape(Q, 3 * prim).copy()

    ran = EA.run_pipelined(groups.items(), p.batch_size, enqueue, read, EA.release_pending)   # source states of at most batch_size crystals of one reps
    EA.settle_saturation(ran, (res["status"] == _lib.VIB_BAD_INPUT).any(), "phonons")
    return res


def analyze_records(p, records):
    """Analyse a list of records on the analysis' mesh: a dict of per-record results, same length, same order -- frequencies (list of
    arrays [Q][3 n], THz, ascending per q; negative: imaginary), n_imag and n_zero (weighted counts over the full mesh), c_v [n][K] (k_B per
    primitive cell), c_v_mol (J / K / mol of primitive cells), c_v_gram (J / K / g), zpe (eV per primitive cell), min_freq and min_q (the
    index into qpoints), asym, herm, pair_gap, sweeps_max, status, reps -- and qpoints [Q][3], weights [Q].  A record the network cannot
    take, one whose supercell would exceed VIB_MAX_ATOMS atoms (never silently shrunk), one of more than PHONON_MAX_PRIM atoms and one whose
    handle is refused come back NaN with status -1; when a state's handle is refused its crystals are analysed one by one."""
    qp = mesh_points(p.mesh)
    return _analyze(p, records, qp, qp.weights)


def band_structure(p, records, qpoints):
    """The frequencies (THz) of every record at an explicit q list -- an array [Q][3] in fractional reciprocal coordinates of the primitive
    cell, or a MeshPoints -- each point with weight 1: a list of arrays [Q][3 n] (empty for a record that was refused)."""
    Q = len(qpoints.k) if isinstance(qpoints, MeshPoints) else len(np.asarray(qpoints, dtype=np.float64).reshape(-1, 3))
    return _analyze(p, records, qpoints, np.ones(Q, np.int32))["frequencies"]
