"""What the analyses of a learned energy share (relax.py, vibrations.py, elasticity.py, phonons.py): the checked configuration,
records -> float32 state, the chunk loop with its handle reuse, and the pipelined driver of a list of records.  The lifetime rules are
stated here once.  A batch handle is made per distinct chunk shape and released only once the stream has passed the work enqueued on
it (a synchronize in front of every release); the plan tensors and buffers of a chunk stay alive in src["keep"] until the state is read;
a state is read behind the next state's enqueue, so two are alive at most; a state whose handle is refused (MIError) is run crystal by
crystal; an error of any other kind releases what is pending and propagates; the process-wide saturation count is settled once, at the
end of a call that ran anything."""
import contextlib
import ctypes as C
import logging

import numpy as np
import torch

from . import _lib


def _at(t):
    """The device address of a contiguous tensor of any element type (the float64 and int64 arrays of the analyses included)."""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), (t.device, t.is_contiguous())
    return C.c_void_p(t.data_ptr())


class EnergyAnalysis:
    """The configuration every analysis starts from: predictor, a PropertyPredictor (fc edge style, clean or noise-aware; the time is 0);
    task: the property read as the energy; per_atom: the property is an energy per atom; batch_size; det_min: the |det L| below which a
    crystal is bad input; delta: the finite-difference step, where the analysis has one.  Refusals are ValueErrors that name the class."""

    def __init__(self, predictor, task, per_atom=True, batch_size=256, det_min=1e-3, delta=None):
        who = type(self).__name__
        if predictor.hparams.get("edge_style", "fc") != "fc":
            raise ValueError(f"{who}: a knn-style predictor has no input gradient (the fully connected pair mode only)")
        if task not in predictor.names:
            raise ValueError(f"{who}: task = {task!r} is not a property of the predictor ({predictor.names})")
        for k, val in (("delta", delta), ("det_min", det_min))[delta is None:]:
            if not (np.isfinite(float(val)) and float(val) > 0):
                raise ValueError(f"{who}: {k} = {val}: must be finite and positive")
        if int(batch_size) < 1:
            raise ValueError(f"{who}: batch_size = {batch_size}: must be >= 1")
        self.predictor, self.task, self.p = predictor, str(task), predictor.names.index(task)
        self.per_atom, self.batch_size, self.det_min = bool(per_atom), int(batch_size), float(det_min)
        if delta is not None:
            self.delta = float(delta)

    def scale(self):
        std = float(self.predictor.normalizer.std[self.p])
        if not (np.isfinite(std) and std > 0):
            raise ValueError(f"{type(self).__name__}: the normaliser's std of {self.task!r} is {std}: the predictor has no fitted normaliser")
        return std

    def __deepcopy__(self, memo):
        return self   # (a config that carries an analysis is merged by copy: the analysis, with its predictor's device handles, is shared)


def pack_records(fields, rows, device, masses=False):
    """The float32 state of the records `rows` of fields (predictor._valid_fields' tuples): (num_atoms, (frac_coords [N][3], lattices
    [B][3][3], atom_types [N][100] one-hot rows) on `device`), and with masses the float64 masses [N] (amu) on the host.  The coordinates
    are wrapped in float64 before the cast."""
    from .structure import MASSES, lattice_matrix
    na = [int(fields[i][0].size) for i in rows]
    z = np.concatenate([fields[i][0] for i in rows])
    types = np.zeros((z.size, _lib.NUM_TYPES), np.float32)
    types[np.arange(z.size), z - 1] = 1.0
    frac = np.concatenate([fields[i][1] for i in rows]) % 1.0
    lat = np.stack([lattice_matrix(fields[i][2], fields[i][3]) for i in rows])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
    state = (up(frac), up(lat), up(types))
    return (na, state, np.asarray(MASSES, dtype=np.float64)[z]) if masses else (na, state)


def gradient_buffers(analysis, Bc, Nc):
    """The float32 arrays of a chunk of Bc copies with Nc atoms: the copies' state, mi_scalar_input_grad's results and its seed (one at the task)."""
    dev, P = analysis.predictor.device, analysis.predictor.P
    e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
    d_out = torch.zeros(Bc, P, device=dev, dtype=torch.float32)
    d_out[:, analysis.p] = 1.0
    return dict(types=e(Nc, _lib.NUM_TYPES), frac=e(Nc, 3), lat=e(Bc, 3, 3), g_frac=e(Nc, 3), g_lat=e(Bc, 3, 3), out=e(Bc, P), d_out=d_out)


def enqueue_chunks(analysis, src, chunks, make_buffers, run):
    """run(handle, plan_src_dev, plan_copy_dev, bufs) for every chunk (src [k] int32, copy [k] int32) of `chunks` on the current stream.
    A chunk whose atom-count list equals the previous chunk's reuses its handle (and its buffers, make_buffers(analysis, Bc, Nc): the stream orders
    the reuse).  Returns the number of chunks."""
    m = analysis.predictor
    m.trunk.sync()
    prev, cb, bufs = None, None, None
    for ps, pc in chunks:
        na = [src["na"][b] for b in ps]
        if na != prev:
            if cb is not None:   # the old handle goes once the stream has passed its work: a wait, not a read (its memory is not held to the end)
                torch.cuda.current_stream().synchronize()
                src["handles"].remove(cb)
                cb.release()
            cb = m.make_batch(na)
            src["handles"].append(cb)   # (the last one is released by release_handles, behind the stream's work)
            bufs = make_buffers(analysis, len(na), sum(na))
            prev = na
        dev_s, dev_c = torch.from_numpy(ps.copy()).to(m.device), torch.from_numpy(pc.copy()).to(m.device)
        src["keep"] += [dev_s, dev_c, bufs]   # (alive until the read)
        run(cb, dev_s, dev_c, bufs)
    return len(chunks)


def release_handles(src):
    for cb in src["handles"]:
        cb.release()
    src["handles"], src["keep"] = [], []


def release_behind_stream(src):
    torch.cuda.current_stream().synchronize()
    release_handles(src)


def release_pending(state):
    """run_pipelined's release of a pending state (rows, ..., src) of the chunked analyses."""
    release_behind_stream(state[-1])


@contextlib.contextmanager
def releasing_on_error(src):
    """analyze_state's guard: on any exception (a refused handle among them) the handles made so far go, behind the work that was enqueued on them."""
    try:
        yield
    except Exception:
        release_behind_stream(src)
        raise


def run_pipelined(groups, batch_size, enqueue, read, release, max_pending=2):
    """Drive enqueue(key, rows) -> state and read(state) over groups, an iterable of (key, rows): every group is cut into states of at
    most batch_size rows, and a state is read once max_pending are enqueued (2: behind the next one's enqueue, so the device stays busy
    and two workspaces are alive at most; None: every read at the end).  A state whose enqueue raises MIError -- a handle was refused,
    nothing of it is left behind -- is enqueued row by row, and a row refused on its own is skipped.  Any other error propagates, with
    release(state) on every state still pending.  Returns whether anything was enqueued."""
    pend, ran = [], False

    def submit(key, rows):
        nonlocal ran
        pend.append(enqueue(key, rows))
        ran = True
        while max_pending is not None and len(pend) >= max_pending:
            read(pend.pop(0))

    try:
        for key, ok in groups:
            for s in range(0, len(ok), batch_size):
                rows = ok[s:s + batch_size]
                try:
                    submit(key, rows)
                except _lib.MIError:
                    for i in rows:
                        try:
                            submit(key, [i])
                        except _lib.MIError:
                            pass
        while pend:
            read(pend.pop(0))
    finally:
        for state in pend:   # (an error other than a refusal: nothing stays allocated)
            release(state)
    return ran


def settle_saturation(ran, any_bad, where, what="chunks that hold bad-input crystals (their results are NaN)"):
    """Operand conversions that left the fp16 plane format's range are counted process-wide: a call that ran anything accounts for its own
    here.  With bad-input or failed crystals among the results (any_bad) a count is logged -- `what` says where they sat -- otherwise it raises."""
    if not ran:
        return
    cnt = _lib.saturation_events(reset=True)
    if cnt and any_bad:
        logging.warning(f"{where}: {cnt} operand conversions saturated in {what}")
    elif cnt:
        _lib.check_saturation_count(cnt, where)
