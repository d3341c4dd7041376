"""Gamma-point vibrations of a learned energy: normal modes, dynamical stability and the harmonic heat capacity on the device
(include/matinvent_hip_vib.h).

The reference's phonon reward (rewards/calculators/fairchem/phonon.py) relaxes a structure, runs a finite-displacement phonon
calculation and returns the heat capacity at 300 K per gram.  Here the energy is one property of a PropertyPredictor (predictor.py), its
gradient the predictor's input gradient (mi_scalar_input_grad), the force convention relax.py's (cart = frac L, dE / dr = s g_frac L^-T),
and the Hessian the central difference of that gradient over the 6 n displaced copies of a crystal of n atoms.  The copies of every crystal
are laid out in one flat list and cut into chunks of batch_size; mi_vib_run_chunk writes a chunk's copies, differentiates them and stores
their Cartesian gradients, float64, in the crystal's workspace.  Behind the last chunk: mi_vib_dynmat (symmetrise, acoustic sum rule,
mass-weight, project the three translations out), mi_sym_eigvals (cyclic Jacobi, one workgroup per matrix), mi_vib_thermo (frequencies in
THz, imaginary and zero counts, c_v(T), the zero-point energy).  Everything is enqueued on the current stream; a source state (at most
batch_size crystals) is read once, behind the next state's enqueue, so two workspaces are alive at most.

supercell = (a, b, c) replicates a record on the host first: Gamma of the supercell samples the commensurate q-points of the cell.  The
displaced set is NOT reduced by the supercell's translation symmetry (every atom of every image is displaced): phonons.py does that.
delta, nu_cut and det_min ship UNTUNED, and no weight of this repository is trained: nothing about the quality of a frequency or a heat
capacity is claimed."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import energy_analysis as EA
from .energy_analysis import _at, release_handles   # noqa: F401  (release_handles follows the read of a state)

STATUS = ("ok", "no_convergence", "bad_input")
KB_J_MOL = 8.31446261815324   # k_B N_A in J / (K mol), CODATA 2018 (both exact)


class HarmonicAnalysis(EA.EnergyAnalysis):
    """An analysis that ends in a thermo launch (Vibrations here, phonons.Phonons): the checked temperatures (a tuple) and nu_cut on top of
    the shared configuration."""

    def __init__(self, predictor, task, delta, per_atom, temperatures, nu_cut, batch_size, det_min):
        super().__init__(predictor, task, per_atom=per_atom, batch_size=batch_size, det_min=det_min, delta=delta)
        who = type(self).__name__
        temps = tuple(float(t) for t in np.atleast_1d(np.asarray(temperatures, dtype=np.float64)))
        if not 1 <= len(temps) <= _lib.VIB_MAX_TEMPS or not all(np.isfinite(t) and t > 0 for t in temps):
            raise ValueError(f"{who}: temperatures = {temperatures}: 1 to {_lib.VIB_MAX_TEMPS} finite positive numbers")
        if not (np.isfinite(float(nu_cut)) and float(nu_cut) >= 0):
            raise ValueError(f"{who}: nu_cut = {nu_cut}: must be finite and >= 0")
        self.temperatures, self.nu_cut = temps, float(nu_cut)


class Vibrations(HarmonicAnalysis):
    """What an analysis needs: predictor, a PropertyPredictor (fc edge style, clean or noise-aware; the time is 0); task: the property read
    as the energy (eV); delta: the displacement h in Angstrom; per_atom: the property is an energy per atom (the Hessian is that of n times
    it); temperatures: up to 8, in K; nu_cut: the |frequency| (THz) at or below which a mode counts as zero; batch_size: displaced copies per
    gradient evaluation; supercell: (a, b, c) replicas analysed in place of each record; det_min: the |det L| below which a crystal is
    bad input."""

    def __init__(self, predictor, task, delta=0.01, per_atom=True, temperatures=(300.0,), nu_cut=0.05, batch_size=256, supercell=(1, 1, 1), det_min=1e-3):
        super().__init__(predictor, task, delta, per_atom, temperatures, nu_cut, batch_size, det_min)
        sc = tuple(int(r) for r in supercell)
        if len(sc) != 3 or min(sc) < 1:
            raise ValueError(f"Vibrations: supercell = {supercell}: three integers >= 1")
        self.supercell = sc


def chunk_plan(num_atoms, batch_size):
    """The displaced copies of crystals of num_atoms atoms, (source crystal, c = 6 i + 2 d + s) in order, cut into chunks of batch_size:
    a list of (src [k] int32, copy [k] int32)."""
    na = np.asarray(num_atoms, dtype=np.int64).reshape(-1)
    src = np.repeat(np.arange(len(na), dtype=np.int32), 6 * na)
    off = np.concatenate([[0], np.cumsum(6 * na)])[:-1]
    copy = (np.arange(len(src), dtype=np.int64) - np.repeat(off, 6 * na)).astype(np.int32)
    bs = int(batch_size)
    return [(src[s:s + bs], copy[s:s + bs]) for s in range(0, len(src), bs)]


def _ws_layout(num_atoms):
    """(bytes, o [B + 1] doubles) of mi_vib_workspace."""
    na = (C.c_int * max(len(num_atoms), 1))(*[int(n) for n in num_atoms])
    off = (C.c_int64 * (len(num_atoms) + 1))()
    nbytes = _lib.load().mi_vib_workspace(na, len(num_atoms), off)
    if nbytes < 0:
        _lib.check(int(nbytes), "mi_vib_workspace")
    return int(nbytes), np.asarray(list(off), dtype=np.int64)


def source_arrays(v, state, num_atoms, masses):
    """The device arrays of an analysis of the state (frac_coords [N][3], lattices [B][3][3], atom_types [N][100] float rows) of crystals
    of num_atoms atoms with masses [N] (amu): the state as float32, the offsets, the workspace and every output."""
    dev = v.predictor.device
    na = [int(n) for n in num_atoms]
    B, N = len(na), int(sum(na))
    x, l, a = state
    f = lambda t: t.to(dev, torch.float32).contiguous()
    nbytes, o = _ws_layout(na)
    n64 = np.asarray(na, dtype=np.int64)
    M = 3 * n64 - 3
    ev_off = np.concatenate([[0], np.cumsum(M)])
    up = lambda arr, dt: torch.from_numpy(np.ascontiguousarray(arr)).to(dt).to(dev)
    e = lambda *s, dt=torch.float64: torch.empty(*s, device=dev, dtype=dt)
    K = len(v.temperatures)
    return dict(frac=f(x), lat=f(l), types=f(a), na=na, B=B, N=N, node_off=up(np.concatenate([[0], np.cumsum(n64)]), torch.int32),
                mass=up(np.asarray(masses, dtype=np.float64), torch.float64), ws=e(max(nbytes // 8, 1)), ws_off=up(o[:-1], torch.int64),
                mat_off=up(o[:-1] + 27 * n64 * n64, torch.int64), work_off=up(o[:-1] + 27 * n64 * n64 + M * M, torch.int64), sizes=up(M, torch.int32),
                ev_off=up(ev_off[:-1], torch.int64), ev_off_host=ev_off, evals=e(max(int(ev_off[-1]), 1)), freqs=e(max(int(ev_off[-1]), 1)),
                asym=e(B), dyn_status=e(B, dt=torch.int32), sweeps=e(B, dt=torch.int32), eig_status=e(B, dt=torch.int32), c_v=e(B, K), zpe=e(B),
                n_imag=e(B, dt=torch.int32), n_zero=e(B, dt=torch.int32), status=e(B, dt=torch.int32), keep=[], handles=[])


def chunk_args(v, src, plan_src, plan_copy, bufs):
    """The C argument block of one chunk (bufs: types, frac, lat, g_frac of the chunk)."""
    return _lib.VibChunkArgs(_at(src["types"]), _at(src["frac"]), _at(src["lat"]), _at(src["node_off"]), src["B"], _at(plan_src), _at(plan_copy),
                             _at(bufs["types"]), _at(bufs["frac"]), _at(bufs["lat"]), _at(bufs["g_frac"]), _at(src["ws"]), _at(src["ws_off"]),
                             v.delta, v.scale(), v.det_min, int(v.per_atom))


chunk_buffers = EA.gradient_buffers


def enqueue_gradients(v, src, chunks=None):
    """Every chunk's mi_vib_run_chunk on the current stream (EA.enqueue_chunks): the workspace's Gc rows of every crystal of `src`.
    chunks: the plan (default: chunk_plan of every atom; phonons.py passes the home atoms' copies alone).  Returns the number of chunks."""
    from .cspnet import _stream
    lib, m = _lib.load(), v.predictor

    def run(cb, dev_s, dev_c, bufs):
        _, W, bias = m.head_slices()
        args = chunk_args(v, src, dev_s, dev_c, bufs)
        _lib.check(lib.mi_vib_run_chunk(m.trunk._h, cb._h, C.byref(args), _at(m.time_freqs), _at(W), _at(bias), m.P, _at(bufs["d_out"]), _at(bufs["out"]),
                                        _at(bufs["g_lat"]), _stream()), "mi_vib_run_chunk")

    chunks = chunk_plan(src["na"], v.batch_size) if chunks is None else chunks
    return EA.enqueue_chunks(v, src, chunks, chunk_buffers, run)


def enqueue_dynmat(v, src):
    from .cspnet import _stream
    a = _lib.VibDynmatArgs(_at(src["ws"]), _at(src["ws_off"]), _at(src["node_off"]), _at(src["mass"]), _at(src["asym"]), _at(src["dyn_status"]), v.delta,
                           src["B"], max(src["na"]) if src["na"] else 1)
    _lib.check(_lib.load().mi_vib_dynmat(C.byref(a), _stream()), "mi_vib_dynmat")


def enqueue_eigvals(v, src, no_lds=0):
    from .cspnet import _stream
    a = _lib.SymEigArgs(_at(src["ws"]), _at(src["mat_off"]), _at(src["sizes"]), _at(src["ws"]), _at(src["work_off"]), _at(src["evals"]), _at(src["ev_off"]),
                        _at(src["sweeps"]), _at(src["eig_status"]), src["B"], max(3 * max(src["na"]) - 3, 0) if src["na"] else 0, int(no_lds))
    _lib.check(_lib.load().mi_sym_eigvals(C.byref(a), _stream()), "mi_sym_eigvals")


def enqueue_thermo(v, src):
    from .cspnet import _stream
    t = (C.c_double * 8)(*(list(v.temperatures) + [0.0] * (8 - len(v.temperatures))))
    a = _lib.VibThermoArgs(_at(src["evals"]), _at(src["ev_off"]), _at(src["sizes"]), _at(src["eig_status"]), _at(src["dyn_status"]), _at(src["freqs"]), _at(src["c_v"]), _at(src["zpe"]),
                           _at(src["n_imag"]), _at(src["n_zero"]), _at(src["status"]), t, v.nu_cut, src["B"], len(v.temperatures))
    _lib.check(_lib.load().mi_vib_thermo(C.byref(a), _stream()), "mi_vib_thermo")


def analyze_state(v, state, num_atoms, masses, no_lds=0):
    """The whole analysis of a state on the current stream, nothing read: the device arrays of source_arrays (freqs and evals ragged at
    ev_off_host; c_v [B][K], zpe, asym, n_imag, n_zero, sweeps, status [B]).  Call release_handles(result) after the read."""
    src = source_arrays(v, state, num_atoms, masses)
    if src["B"] == 0:
        return src
    with EA.releasing_on_error(src):
        enqueue_gradients(v, src)
        enqueue_dynmat(v, src)
        enqueue_eigvals(v, src, no_lds)
        enqueue_thermo(v, src)
    return src


def analyze_records(v, records):
    """Analyse a list of records (CrystalData, SimpleStructure, read_extxyz frames, pymatgen structures): a dict of per-record results, same
    length, same order -- frequencies (list of arrays, THz, ascending; negative: imaginary), n_imag, n_zero, c_v [n][K] (k_B), c_v_mol
    (J / K / mol of cells), c_v_gram (J / K / g), zpe (eV), asym, sweeps, status.  A record the network cannot take, one with more than
    VIB_MAX_ATOMS atoms (after the supercell), one that cannot be replicated and one whose handle is refused come back NaN with status -1;
    when a state's handle is refused its crystals are analysed one by one."""
    from .predictor import _valid_fields
    from .structure import make_supercell
    dev = v.predictor.device
    records = list(records)
    n, K = len(records), len(v.temperatures)
    if v.supercell != (1, 1, 1):
        def rep(r):
            try:
                return make_supercell(r, v.supercell)
            except (AttributeError, TypeError, ValueError, IndexError):
                return None   # not a crystal: never analysed in its unreplicated form
        records = [rep(r) for r in records]
    res = dict(frequencies=[np.zeros(0) for _ in range(n)], n_imag=np.full(n, -1, np.int64), n_zero=np.full(n, -1, np.int64), c_v=np.full((n, K), np.nan),
               c_v_mol=np.full((n, K), np.nan), c_v_gram=np.full((n, K), np.nan), zpe=np.full(n, np.nan), asym=np.full(n, np.nan),
               sweeps=np.full(n, -1, np.int64), status=np.full(n, -1, np.int64))
    fields = [None if r is None else _valid_fields(r) for r in records]
    ok = [i for i, f in enumerate(fields) if f is not None and f[0].size <= _lib.VIB_MAX_ATOMS]

    def enqueue(_, rows):
        na, state, mass = EA.pack_records(fields, rows, dev, masses=True)
        return rows, na, mass, analyze_state(v, state, na, mass)   # (MIError: a handle was refused; nothing is left behind)

    def read(st):
        rows, na, mass, src = st
        small = torch.cat([src["c_v"], src["zpe"][:, None], src["asym"][:, None]] +
                          [src[k].to(torch.float64)[:, None] for k in ("n_imag", "n_zero", "sweeps", "status")], dim=1).cpu().numpy()
        freqs = src["freqs"].cpu().numpy()
        release_handles(src)
        off, eo = np.concatenate([[0], np.cumsum(na)]), src["ev_off_host"]
        for k, i in enumerate(rows):
            res["c_v"][i] = small[k, :K]
            res["c_v_mol"][i] = small[k, :K] * KB_J_MOL
            res["c_v_gram"][i] = small[k, :K] * KB_J_MOL / mass[off[k]:off[k + 1]].sum()
            res["zpe"][i], res["asym"][i] = small[k, K], small[k, K + 1]
            res["n_imag"][i], res["n_zero"][i], res["sweeps"][i], res["status"][i] = (int(small[k, K + 2 + j]) for j in range(4))
            res["frequencies"][i] = freqs[eo[k]:eo[k + 1]].copy()

    ran = EA.run_pipelined([(None, ok)], v.batch_size, enqueue, read, EA.release_pending)   # source states of at most batch_size crystals
    EA.settle_saturation(ran, (res["status"] == _lib.VIB_BAD_INPUT).any(), "analyze_records")
    return res
