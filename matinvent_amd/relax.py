"""Batched structure relaxation on a learned energy: FIRE on the device (include/matinvent_hip_relax.h).

The reference's sample step relaxes before it filters and scores (pipeline/mat_invent.py:88-91: sample_cfg.mlip_opt(strucs, xyz_path) ->
(relaxed structures, energies); pipeline/filters/opt_filter.py: MatterSim, FIRE with a cell filter).  Here the energy is one property of
a PropertyPredictor (predictor.py), its forces are the predictor's input gradient (mi_scalar_input_grad) on the state's own arrays, and one
FIRE step is one small launch behind it (mi_relax_step): mi_relax_run enqueues `steps` such pairs on the current stream and the host reads
nothing until the end.  Lattice rows are cell vectors, cart = frac L:  F_i = -s g_frac[i] L^-T and, with relax_cell, F_L = -s g_lat / c, with
s = std (x n when the property is per atom) and c = cell_factor (default: the atom count, as ASE's cell filters).  fmax is in the property's
raw unit per Angstrom.  A clean or a noise-aware predictor is taken; the time is 0.  cell_factor, fmax and steps ship UNTUNED, and no weight
of this repository is trained: nothing about the quality of a relaxed structure is claimed.  A crystal that has converged or failed is
frozen bit for bit but still rides through every gradient evaluation of its batch (no compaction)."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import energy_analysis as EA

STATUS = ("active", "converged", "failed", "exhausted")
FIRE_DEFAULTS = dict(dt=0.1, dt_max=1.0, maxstep=0.2, n_min=5, f_inc=1.1, f_dec=0.5, a_start=0.1, f_a=0.99)   # ASE's FIRE
_POSITIVE = ("fmax", "dt", "dt_max", "maxstep", "f_inc", "f_dec", "a_start", "f_a")


class Relaxer(EA.EnergyAnalysis):
    """What a relaxation needs: predictor, a PropertyPredictor (fc edge style, clean or noise-aware); task: the property read as the
    energy; steps: FIRE steps per crystal at most; fmax: the convergence threshold on the largest force row (raw unit per Angstrom);
    relax_cell: the lattice moves too (three more rows of force, -s g_lat / c); per_atom: the property is an energy per atom (the forces
    are those of n times it); cell_factor: c, None = the crystal's atom count; check_every = k > 0: the host reads the number of active
    crystals every k steps and stops early (0: never waits); batch_size: crystals per handle of relax_records; det_min: the |det L| below
    which a crystal fails; the remaining keywords are FIRE's constants.  Callable as the reference's mlip_opt:
    relaxer(strucs, xyz_path=None) -> (strucs, energies)."""

    def __init__(self, predictor, task, steps=50, fmax=0.1, relax_cell=True, per_atom=True, cell_factor=None, check_every=0, batch_size=64,
                 det_min=1e-3, **fire):
        super().__init__(predictor, task, per_atom=per_atom, batch_size=batch_size, det_min=det_min)
        unknown = set(fire) - set(FIRE_DEFAULTS)
        if unknown:
            raise ValueError(f"Relaxer: unknown keywords {sorted(unknown)}")
        v = dict(FIRE_DEFAULTS, **fire, fmax=fmax, det_min=self.det_min)
        for k in _POSITIVE:
            if not (np.isfinite(float(v[k])) and float(v[k]) > 0):
                raise ValueError(f"Relaxer: {k} = {v[k]}: must be finite and positive")
        if int(v["n_min"]) < 0:
            raise ValueError(f"Relaxer: n_min = {v['n_min']}: must be >= 0")
        if int(steps) < 0:
            raise ValueError(f"Relaxer: steps = {steps}: must be >= 0")
        if int(check_every) < 0:
            raise ValueError(f"Relaxer: check_every = {check_every}: 0 (never wait for the host) or a positive number of steps")
        if cell_factor is not None and not (np.isfinite(float(cell_factor)) and float(cell_factor) > 0):
            raise ValueError(f"Relaxer: cell_factor = {cell_factor}: None (the crystal's atom count) or a positive number")
        self.steps, self.check_every, self.relax_cell = int(steps), int(check_every), bool(relax_cell)
        self.cell_factor = None if cell_factor is None else float(cell_factor)
        self.fire = {k: (int(v[k]) if k == "n_min" else float(v[k])) for k in list(FIRE_DEFAULTS) + ["fmax", "det_min"]}
        self.last_info = None

    def params(self):
        """The C parameter block: the constants, and scale = the normaliser's std of the task."""
        f = self.fire
        return _lib.RelaxParams(f["dt"], f["dt_max"], f["maxstep"], f["f_inc"], f["f_dec"], f["a_start"], f["f_a"], f["fmax"], self.scale(),
                                0.0 if self.cell_factor is None else self.cell_factor, f["det_min"], f["n_min"], int(self.relax_cell), int(self.per_atom))

    def __call__(self, strucs, xyz_path=None):
        return relax_records(self, strucs)

    @classmethod
    def from_config(cls, spec, device=None):
        """sample_cfg.mlip_opt: a callable (returned as it is), None, or a mapping {model_path, task, ...Relaxer's keywords} whose predictor
        is read with predictor.load_predictor."""
        if spec is None or callable(spec):
            return spec
        from .predictor import load_predictor
        d = {str(k): v for k, v in dict(spec).items()}
        if not d.get("model_path") or not d.get("task"):
            raise ValueError("sample_cfg.mlip_opt needs model_path (a directory written by save_predictor) and task")
        pred = load_predictor(str(d.pop("model_path")), device=device)
        return cls(pred, **d)


def relax_buffers(relaxer, B, N, device):
    """The device arrays of one relaxation: velocities, the two state blocks, the seed, and mi_scalar_input_grad's three results."""
    P = relaxer.predictor.P
    e = lambda *s, dt=torch.float32: torch.empty(*s, device=device, dtype=dt)
    return dict(vel_x=e(N, 3), vel_l=e(B, 3, 3), fs=e(B, _lib.RELAX_NF), is_=e(B, _lib.RELAX_NI, dt=torch.int32), d_out=e(B, P), out=e(B, P),
                g_frac=e(N, 3), g_lat=e(B, 3, 3))


def relax_enqueue(relaxer, state, handle, bufs=None, steps=None):
    """mi_relax_init and mi_relax_run on the current stream, IN PLACE on state = (frac_coords, lattices, atom_types) (float32, contiguous,
    on the predictor's device; the type rows are read only).  Returns the buffers (relax_buffers); nothing is read unless check_every > 0."""
    from .cspnet import _ptr, _stream
    lib = _lib.load()
    m = relaxer.predictor
    x, l, a = state
    B, N, P = handle.num_graphs, handle.num_nodes, m.P
    if a.numel() != N * _lib.NUM_TYPES or x.numel() != N * 3 or l.numel() != B * 9:
        raise ValueError(f"relax_state: the state's shapes {tuple(a.shape)}, {tuple(x.shape)}, {tuple(l.shape)} are not the handle's {N} atoms in {B} crystals")
    bufs = relax_buffers(relaxer, B, N, m.device) if bufs is None else bufs
    prm = relaxer.params()
    steps = relaxer.steps if steps is None else int(steps)
    m.trunk.sync()
    _, W, bias = m.head_slices()
    _lib.check(lib.mi_relax_init(handle._h, C.byref(prm), P, relaxer.p, _ptr(bufs["vel_x"]), _ptr(bufs["vel_l"]), _ptr(bufs["fs"]), _ptr(bufs["is_"]),
                                 _ptr(bufs["d_out"]), _stream()), "mi_relax_init")

    def run(k, finish):
        _lib.check(lib.mi_relax_run(m.trunk._h, handle._h, C.byref(prm), _ptr(a), _ptr(x), _ptr(l), _ptr(m.time_freqs), _ptr(W), _ptr(bias), P, relaxer.p,
                                    _ptr(bufs["d_out"]), _ptr(bufs["out"]), _ptr(bufs["g_frac"]), _ptr(bufs["g_lat"]), _ptr(bufs["vel_x"]),
                                    _ptr(bufs["vel_l"]), _ptr(bufs["fs"]), _ptr(bufs["is_"]), int(k), int(finish), _stream()), "mi_relax_run")

    if relaxer.check_every <= 0:
        run(steps, 1)
        return bufs
    done = 0
    while done < steps:
        k = min(relaxer.check_every, steps - done)
        done += k
        run(k, 1 if done == steps else 0)
        if done < steps and int((bufs["is_"][:, 0] == _lib.RELAX_ACTIVE).sum()) == 0:   # (the read of the active count)
            break
    return bufs


def read_info(relaxer, bufs, num_atoms):
    """The call's one read: status [B] ints (and their names), steps, the first and last energy in raw units (the property's own: per atom
    when per_atom), the last largest force row and the last |dr|."""
    host = torch.cat([bufs["fs"], bufs["is_"].to(torch.float32)], dim=1).cpu().double().numpy()   # (small ints: exact in float32)
    nm = relaxer.predictor.normalizer
    mean, std = float(nm.mean[relaxer.p]), float(nm.std[relaxer.p])
    status = host[:, _lib.RELAX_NF].astype(np.int64)
    none = (status == _lib.RELAX_FAILED) | (status == _lib.RELAX_ACTIVE)   # (failed, or -- steps = 0 -- never evaluated)
    raw = lambda col: np.where(none, np.nan, host[:, col] * std + mean)
    return dict(status=status, status_names=[STATUS[s] for s in status], steps=host[:, _lib.RELAX_NF + 2].astype(np.int64), e_first=raw(2), e_last=raw(3),
                fmax=host[:, 4], dr=host[:, 5], dt=host[:, 0], num_atoms=np.asarray(num_atoms, np.int64))


def relax_state(relaxer, state, handle):
    """Relax a state -- a dict with atom_types [N][100] float rows, frac_coords [N][3], lattices [B][3][3], or the tuple (frac_coords,
    lattices, atom_types) -- on `handle`, a batch handle of the relaxer's predictor with the state's atom counts.  The caller's arrays are
    left unchanged.  Returns (the relaxed state in the caller's form, info): info from read_info, the call's one read at its end."""
    dev = relaxer.predictor.device
    as_dict = isinstance(state, dict)
    x, l, a = (state["frac_coords"], state["lattices"], state["atom_types"]) if as_dict else state
    f = lambda v: v.to(dev, torch.float32).contiguous()
    x, l, a = f(x).clone(), f(l).clone(), f(a)
    bufs = relax_enqueue(relaxer, (x, l, a), handle)
    info = read_info(relaxer, bufs, handle.num_atoms_list)
    out = dict(state, frac_coords=x, lattices=l, atom_types=a) if as_dict else (x, l, a)
    return out, info


def _lengths_angles(L):
    """(lengths [3], angles [3] in degrees) of a 3 x 3 matrix of cell rows: the Gram matrix L L^T read back."""
    G = L @ L.T
    le = np.sqrt(np.diag(G))
    cos = [G[(k + 1) % 3, (k + 2) % 3] / (le[(k + 1) % 3] * le[(k + 2) % 3]) for k in range(3)]
    return le.tolist(), [float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))) for c in cos]


def relax_records(relaxer, records):
    """Relax a list of records (CrystalData, SimpleStructure, read_extxyz frames, pymatgen structures) in batches of relaxer.batch_size:
    -> (structures, energies).  Same length, same order.  A relaxed record is a data.SimpleStructure with the relaxed coordinates and
    lengths / angles from the relaxed matrix; its energy (float64, the property's raw unit) is the last evaluated one.  A crystal that
    FAILED, a record the network cannot take and a record whose handle is refused come back as they were, with energy NaN.
    relaxer.last_info: per record status (-1: never ran), steps, first energy."""
    from .data import SimpleStructure
    from .predictor import _valid_fields
    m = relaxer.predictor
    dev = m.device
    records = list(records)
    n = len(records)
    out, energies = list(records), np.full(n, np.nan, dtype=np.float64)
    last = dict(status=np.full(n, -1, np.int64), steps=np.zeros(n, np.int64), e_first=np.full(n, np.nan), fmax=np.full(n, np.nan))
    fields = [_valid_fields(r) for r in records]
    ok = [i for i, f in enumerate(fields) if f is not None]

    def enqueue(_, rows):
        cb = m.make_batch([int(fields[i][0].size) for i in rows])   # (MIError: an atom count the handle refuses)
        try:
            na, st = EA.pack_records(fields, rows, dev)
            bufs = relax_enqueue(relaxer, st, cb)
        except Exception:
            cb.release()
            raise
        return rows, na, cb, st, bufs

    def read(state):
        rows, na, cb, st, bufs = state
        info = read_info(relaxer, bufs, na)
        x, l = st[0].cpu().double().numpy(), st[1].cpu().double().numpy()
        cb.release()
        off = np.concatenate([[0], np.cumsum(na)])
        for k, i in enumerate(rows):
            last["status"][i], last["steps"][i], last["e_first"][i], last["fmax"][i] = info["status"][k], info["steps"][k], info["e_first"][k], info["fmax"][k]
            if info["status"][k] == _lib.RELAX_FAILED or not (np.isfinite(x[off[k]:off[k + 1]]).all() and np.isfinite(l[k]).all()):
                continue
            le, an = _lengths_angles(l[k])
            out[i] = SimpleStructure(le, an, [int(v) for v in fields[i][0]], x[off[k]:off[k + 1]].copy())
            energies[i] = info["e_last"][k]

    def release(state):
        torch.cuda.current_stream().synchronize()
        state[2].release()

    # every batch holds its own handle and nothing is read before the last enqueue (max_pending = None): the reads, behind every batch's work
    ran = EA.run_pipelined([(None, ok)], relaxer.batch_size, enqueue, read, release, max_pending=None)
    EA.settle_saturation(ran, (last["status"] == _lib.RELAX_FAILED).any(), "relax_records", "batches that hold failed crystals (their energies are NaN)")
    relaxer.last_info = last
    return out, energies


def log_metrics(relaxer, energies):
    """The four log keys of a pipeline's relaxation from relaxer.last_info (a plain callable without it: counts from the energies alone)."""
    info = getattr(relaxer, "last_info", None)
    e = np.asarray(energies, dtype=np.float64)
    if info is None or len(info["status"]) != len(e):
        return dict(relax_converged=float("nan"), relax_failed=int((~np.isfinite(e)).sum()), relax_steps_mean=float("nan"), relax_de_mean=float("nan"))
    ran = info["status"] >= 0
    de = (e - info["e_first"])[np.isfinite(e) & np.isfinite(info["e_first"])]
    return dict(relax_converged=int((info["status"] == _lib.RELAX_CONVERGED).sum()), relax_failed=int((~np.isfinite(e)).sum()),
                relax_steps_mean=float(info["steps"][ran].mean()) if ran.any() else float("nan"), relax_de_mean=float(de.mean()) if de.size else float("nan"))
