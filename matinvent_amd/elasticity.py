"""The elastic tensor and moduli of a learned energy on the device (include/matinvent_hip_elastic.h).

The reference's elastic reward (rewards/calculators/fairchem/elastic.py) strains the cell, relaxes the ions in every strained copy, reads
the stresses, fits the tensor and returns the Voigt bulk modulus.  Here the energy is one property of a PropertyPredictor (predictor.py),
its lattice gradient the other half of the predictor's input gradient (mi_scalar_input_grad's g_lat), the convention relax.py's
(cart = frac L, lattice rows are cell vectors), and the stress of a cell sigma = sym(L^T G) / V.  Every crystal has 13 copies whatever its
size -- twelve strained by +-delta along the six Voigt components and the unstrained one -- laid out in one flat list and cut into chunks
of batch_size; mi_elastic_run_chunk writes a chunk's copies, relaxes their ions at the fixed strained cell for ion_steps FIRE steps when
asked to, differentiates them and stores their stresses, float64, in the crystal's 13 x 8 workspace rows.  Behind the last chunk
mi_elastic_fit forms C (GPa) by central differences, S = C^-1, the Voigt / Reuss / Hill averages of K and G with Young's modulus,
Poisson's ratio and the Pugh ratio of each, the eigenvalues of C, the count of negative ones (Born stability) and the condition number.
Everything is enqueued on the current stream; a source state (at most batch_size crystals) is read once, behind the next state's enqueue.

C is the derivative of the Cauchy stress at the GIVEN structure: under a residual stress it is not the energy's second derivative, which
is why stress0 and pressure come back too (relax the structure first when that matters).  delta, det_min and the FIRE constants of the
ion relaxation ship UNTUNED, and no weight of this repository is trained: nothing about the quality of a modulus is claimed."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import energy_analysis as EA
from .energy_analysis import _at, release_handles   # noqa: F401  (release_handles follows the read of a state)
from .relax import FIRE_DEFAULTS

STATUS = ("ok", "bad_input", "singular")
AVERAGES = ("voigt", "reuss", "hill")
MODULI = ("bulk_modulus", "shear_modulus", "young_modulus", "poisson_ratio", "pugh_ratio")   # the columns of moduli [3][5]
_FIT = (("C", 36), ("S", 36), ("stress0", 6), ("pressure", 1), ("asym", 1), ("asym_C", 1), ("moduli", 15), ("evals", 6), ("cond", 1))
_COUNTS = ("n_negative", "n_unrelaxed", "status")


class Elasticity(EA.EnergyAnalysis):
    """What an analysis needs: predictor, a PropertyPredictor (fc edge style, clean or noise-aware; the time is 0); task: the property read
    as the energy (eV); delta: the strain h (untuned); per_atom: the property is an energy per atom (the stress is that of n times it);
    ion_steps: FIRE steps of the ions in every strained copy at its fixed cell (0: the ions are clamped at their fractional coordinates);
    relax: a dict of Relaxer-style FIRE constants and fmax for that relaxation; batch_size: strained copies per gradient evaluation and
    source crystals per state; det_min: the |det L| below which a crystal is bad input."""

    def __init__(self, predictor, task, delta=0.005, per_atom=True, ion_steps=0, relax=None, batch_size=256, det_min=1e-3):
        super().__init__(predictor, task, per_atom=per_atom, batch_size=batch_size, det_min=det_min, delta=delta)
        if int(ion_steps) < 0:
            raise ValueError(f"Elasticity: ion_steps = {ion_steps}: must be >= 0")
        relax = dict(relax or {})
        unknown = set(relax) - set(FIRE_DEFAULTS) - {"fmax"}
        if unknown:
            raise ValueError(f"Elasticity: unknown relax keywords {sorted(unknown)}")
        fire = {**FIRE_DEFAULTS, "fmax": 0.1, **relax}
        for k, val in fire.items():
            if k == "n_min":
                if int(val) < 0:
                    raise ValueError(f"Elasticity: n_min = {val}: must be >= 0")
            elif not (np.isfinite(float(val)) and float(val) > 0):
                raise ValueError(f"Elasticity: {k} = {val}: must be finite and positive")
        self.ion_steps = int(ion_steps)
        self.fire = {k: (int(v) if k == "n_min" else float(v)) for k, v in fire.items()}

    def relax_params(self):
        """The C parameter block of the ion relaxation (relax_cell, scale, det_min and per_atom are the chunk's own: mi_elastic_run_chunk)."""
        f = self.fire
        return _lib.RelaxParams(f["dt"], f["dt_max"], f["maxstep"], f["f_inc"], f["f_dec"], f["a_start"], f["f_a"], f["fmax"], self.scale(), 0.0,
                                self.det_min, f["n_min"], 0, int(self.per_atom))


def chunk_plan(num_crystals, batch_size):
    """The strained copies of num_crystals crystals, (source crystal, c = 2 j + s; 12: unstrained) in order, cut into chunks of batch_size:
    a list of (src [k] int32, copy [k] int32)."""
    B = int(num_crystals)
    src = np.repeat(np.arange(B, dtype=np.int32), _lib.ELASTIC_COPIES)
    copy = np.tile(np.arange(_lib.ELASTIC_COPIES, dtype=np.int32), B)
    bs = int(batch_size)
    return [(src[s:s + bs], copy[s:s + bs]) for s in range(0, len(src), bs)]


def source_arrays(e, state, num_atoms):
    """The device arrays of an analysis of the state (frac_coords [N][3], lattices [B][3][3], atom_types [N][100] float rows) of crystals
    of num_atoms atoms: the state as float32, the offsets, the workspace and every output."""
    dev = e.predictor.device
    na = [int(n) for n in num_atoms]
    B, N = len(na), int(sum(na))
    x, l, a = state
    f = lambda t: t.to(dev, torch.float32).contiguous()
    node_off = torch.from_numpy(np.concatenate([[0], np.cumsum(np.asarray(na, dtype=np.int64))]).astype(np.int32)).to(dev)
    d = lambda *s, dt=torch.float64: torch.empty(*s, device=dev, dtype=dt)
    out = dict(frac=f(x), lat=f(l), types=f(a), na=na, B=B, N=N, node_off=node_off, ws=d(max(B, 1), _lib.ELASTIC_COPIES, _lib.ELASTIC_ROW), keep=[], handles=[])
    for k, w in _FIT:
        out[k] = d(B, w) if w > 1 else d(B)
    for k in _COUNTS:
        out[k] = d(B, dt=torch.int32)
    return out


def chunk_buffers(e, Bc, Nc):
    """EA.gradient_buffers and the state of the ion relaxation."""
    dev = e.predictor.device
    f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
    return dict(EA.gradient_buffers(e, Bc, Nc), vel_x=f(Nc, 3), fstate=f(Bc, _lib.RELAX_NF), istate=torch.empty(Bc, _lib.RELAX_NI, device=dev, dtype=torch.int32))


def chunk_args(e, src, plan_src, plan_copy, bufs, relaxed=None):
    """The C argument block of one chunk (bufs: chunk_buffers); relaxed: istate is handed to the collect step (None: when ion_steps > 0)."""
    relaxed = e.ion_steps > 0 if relaxed is None else relaxed
    return _lib.ElasticChunkArgs(_at(src["types"]), _at(src["frac"]), _at(src["lat"]), _at(src["node_off"]), src["B"], _at(plan_src), _at(plan_copy),
                                 _at(bufs["types"]), _at(bufs["frac"]), _at(bufs["lat"]), _at(bufs["g_frac"]), _at(bufs["g_lat"]),
                                 _at(bufs["istate"]) if relaxed else None, _at(src["ws"]), _at(src["asym"]), e.delta, e.scale(), e.det_min, int(e.per_atom))


def run_chunk(e, handle, args, bufs):
    """mi_elastic_run_chunk of one chunk on the current stream."""
    from .cspnet import _stream
    m = e.predictor
    _, W, bias = m.head_slices()
    rp = e.relax_params()
    _lib.check(_lib.load().mi_elastic_run_chunk(m.trunk._h, handle._h, C.byref(args), C.byref(rp), e.ion_steps, _at(m.time_freqs), _at(W), _at(bias), m.P,
                                                e.p, _at(bufs["d_out"]), _at(bufs["out"]), _at(bufs["vel_x"]), _at(bufs["fstate"]), _stream()),
               "mi_elastic_run_chunk")


def enqueue_stresses(e, src):
    """Every chunk's mi_elastic_run_chunk on the current stream (EA.enqueue_chunks): the workspace rows of every crystal of `src`.
    Returns the number of chunks."""
    return EA.enqueue_chunks(e, src, chunk_plan(src["B"], e.batch_size), chunk_buffers,
                             lambda cb, dev_s, dev_c, bufs: run_chunk(e, cb, chunk_args(e, src, dev_s, dev_c, bufs), bufs))


def fit_args(e, src):
    return _lib.ElasticFitArgs(_at(src["ws"]), *[_at(src[k]) for k, _ in _FIT], *[_at(src[k]) for k in _COUNTS], e.delta, src["B"])


def enqueue_fit(e, src):
    from .cspnet import _stream
    a = fit_args(e, src)
    _lib.check(_lib.load().mi_elastic_fit(C.byref(a), _stream()), "mi_elastic_fit")


def analyze_state(e, state, num_atoms):
    """The whole analysis of a state on the current stream, nothing read: the device arrays of source_arrays (C, S [B][36], stress0 [B][6],
    moduli [B][15], evals [B][6], pressure, asym, asym_C, cond, n_negative, n_unrelaxed, status [B]).  Call release_handles(result) after
    the read."""
    src = source_arrays(e, state, num_atoms)
    if src["B"] == 0:
        return src
    with EA.releasing_on_error(src):
        enqueue_stresses(e, src)
        enqueue_fit(e, src)
    return src


def empty_results(n):
    res = {k: np.full((n, w) if w > 1 else n, np.nan) for k, w in _FIT}
    res["C"], res["S"], res["moduli"] = res["C"].reshape(n, 6, 6), res["S"].reshape(n, 6, 6), res["moduli"].reshape(n, 3, 5)
    for k in _COUNTS:
        res[k] = np.full(n, -1, np.int64)
    return res


def add_shortcuts(res):
    """bulk_modulus, shear_modulus, young_modulus, poisson_ratio and pugh_ratio as [n][3] over Voigt / Reuss / Hill."""
    for j, name in enumerate(MODULI):
        res[name] = res["moduli"][:, :, j].copy()
    return res


def analyze_records(e, records):
    """Analyse a list of records (CrystalData, SimpleStructure, read_extxyz frames, pymatgen structures): a dict of per-record results, same
    length, same order -- C, S [n][6][6] (GPa, 1 / GPa), stress0 [n][6], pressure (GPa), asym, asym_C, moduli [n][3][5], evals [n][6], cond,
    n_negative, n_unrelaxed, status, and the shortcuts bulk_modulus, shear_modulus, young_modulus, pugh_ratio, poisson_ratio [n][3] over
    Voigt / Reuss / Hill.  A record the network cannot take and one whose handle is refused come back NaN with status -1; when a state's
    handle is refused its crystals are analysed one by one."""
    from .predictor import _valid_fields
    dev = e.predictor.device
    records = list(records)
    n = len(records)
    res = empty_results(n)
    fields = [_valid_fields(r) for r in records]
    ok = [i for i, f in enumerate(fields) if f is not None]
    widths = [w for _, w in _FIT]

    def enqueue(_, rows):
        na, state = EA.pack_records(fields, rows, dev)
        return rows, analyze_state(e, state, na)   # (MIError: a handle was refused; nothing is left behind)

    def read(st):
        rows, src = st
        B = src["B"]
        flat = torch.cat([src[k].reshape(B, -1) for k, _ in _FIT] + [src[k].to(torch.float64)[:, None] for k in _COUNTS], dim=1).cpu().numpy()
        release_handles(src)
        at = 0
        for k, w in _FIT:
            res[k][rows] = flat[:, at:at + w].reshape((B,) + res[k].shape[1:])
            at += w
        for j, k in enumerate(_COUNTS):
            res[k][rows] = flat[:, at + j].astype(np.int64)

    ran = EA.run_pipelined([(None, ok)], e.batch_size, enqueue, read, EA.release_pending)   # source states of at most batch_size crystals
    EA.settle_saturation(ran, (res["status"] == _lib.ELASTIC_BAD_INPUT).any(), "analyze_records")
    return add_shortcuts(res)
