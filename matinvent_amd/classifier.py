"""Classifier guidance of the reverse chain from the property predictor's input gradient (include/matinvent_hip_inputgrad.h).

Dhariwal & Nichol's Algorithm 1: the mean of the transition x_t -> x_{t-1} is shifted by scale * Sigma_t * grad log p(y | x_t), the
gradient taken at x_t.  Here p(y | x_t) comes from a NOISE-AWARE property predictor (predictor.fit_predictor(diffusion=)):
log p = +out ("max"), -out ("min") or the unit-width Gaussian -(out - target)^2 / 2 ("target"; the width lives in `scale`), in the
predictor's normalised units.  The shift is applied to the lattice's and the type rows' DDPM step with Sigma_t = sigma_t^2, and to the
coordinates' Langevin corrector plus predictor as ONE gradient per step with Sigma_t = step_corr + step_pred (the corrector's midpoint is
not re-evaluated).

The chain is walked step by step inside the guided window: mi_scalar_input_grad at x_t on a handle of the predictor's own, ONE single-step
mi_sampler_run segment, mi_guide_shift with the step's coefficients.  Everything is enqueued on the current stream; the host reads
nothing until the chain has ended.  `scale` is untuned."""
import ctypes as C

import numpy as np
import torch

from . import _lib

MODES = ("max", "min", "target")
C_STEP_CORR, C_STEP_PRED, C_SIGMA2 = 4, 6, 10   # columns of DiffCSPModule._coefficients (include/matinvent_hip.h: MI_C_*)


def refuse(where, **keys):
    """A shifted chain's recorded log-probabilities would be the unshifted proposal's: sample_mdp / sample_rollout / MatInventPG refuse the key."""
    for k, v in keys.items():
        if v is not None:
            raise ValueError(f"{where}: {k} is not supported -- a classifier-guided chain shifts every step's mean, and its recorded "
                             "log-probabilities would be the unshifted proposal's (DESIGN 44)")


class ClassifierGuidance:
    """What a classifier-guided chain needs besides the prior.  predictor: a noise-aware PropertyPredictor (fc edge style); task: one of its
    property names; mode: "max" / "min" / "target" (then target = the raw property value aimed at); scale = s, the guidance scale in the
    predictor's NORMALISED units (untuned); max_shift: None, or the elementwise clamp of every |a g|; the steps t -> t - 1 with
    stop < t <= start are guided (start = None: from the chain's first step); guide_types: the type rows are shifted too."""

    def __init__(self, predictor, task, mode="max", target=None, scale=1.0, max_shift=None, start=None, stop=0, guide_types=False):
        from .predictor import require_noised
        require_noised(predictor, "ClassifierGuidance")
        if predictor.hparams.get("edge_style", "fc") != "fc":
            raise ValueError("ClassifierGuidance: a knn-style predictor has no input gradient (the fully connected pair mode only)")
        if task not in predictor.names:
            raise ValueError(f"ClassifierGuidance: task = {task!r} is not a property of the predictor ({predictor.names})")
        if mode not in MODES:
            raise ValueError(f"ClassifierGuidance: mode = {mode!r}: it takes 'max', 'min' or 'target'")
        if (mode == "target") != (target is not None):
            raise ValueError("ClassifierGuidance: target = goes with mode = 'target', and only with it")
        if target is not None and not np.isfinite(float(target)):
            raise ValueError(f"ClassifierGuidance: target = {target} is not finite")
        if not np.isfinite(float(scale)):
            raise ValueError(f"ClassifierGuidance: scale = {scale} is not finite")
        if max_shift is not None and not (np.isfinite(float(max_shift)) and float(max_shift) > 0):
            raise ValueError(f"ClassifierGuidance: max_shift = {max_shift}: None (no clamp) or a positive number")
        if start is not None and int(start) < 1:
            raise ValueError(f"ClassifierGuidance: start = {start}: None (the chain's first step) or a step index >= 1")
        if int(stop) < 0 or (start is not None and int(stop) >= int(start)):
            raise ValueError(f"ClassifierGuidance: stop = {stop}: 0 <= stop < start")
        self.predictor, self.task, self.mode = predictor, str(task), mode
        self.p = predictor.names.index(task)
        self.target = None if target is None else float(target)
        self.scale = float(scale)
        self.max_shift = None if max_shift is None else float(max_shift)
        self.start = None if start is None else int(start)
        self.stop = int(stop)
        self.guide_types = bool(guide_types)
        self._handles = {}

    def window(self, t_start, t_stop=0):
        """The guided steps of a chain from t_start down to t_stop, descending: the t with max(stop, t_stop) < t <= min(start, t_start) (the
        step t -> t - 1).  On a respaced view these are indices of the view's own grid."""
        hi = int(t_start) if self.start is None else min(self.start, int(t_start))
        lo = max(self.stop, int(t_stop))
        return list(range(hi, lo, -1))

    def coefficients(self, module, step_lr, t):
        """(a_t, a_x, a_l) of the step t -> t - 1 from module._coefficients(step_lr): a_l = scale sigma_t^2, a_t = the same when the type rows
        are guided (else 0: they are left alone), a_x = scale (step_corr + step_pred).  Separately rounded float32, as the host hands them
        to mi_guide_shift."""
        row = module._coefficients(step_lr)[int(t)]
        s = np.float32(self.scale)
        a_l = np.float32(s * np.float32(row[C_SIGMA2]))
        a_x = np.float32(s * np.float32(np.float32(row[C_STEP_CORR]) + np.float32(row[C_STEP_PRED])))
        return (float(a_l) if self.guide_types else 0.0), float(a_x), float(a_l)

    def handle(self, na, node_offset=0, graph_offset=0):
        """The predictor's own batch handle for these atom counts and offsets (a small cache: the chain's handle is never used)."""
        key = (tuple(na), int(node_offset), int(graph_offset))
        h = self._handles.get(key)
        if h is None:
            if len(self._handles) >= 4:
                self._handles.pop(next(iter(self._handles))).release()
            h = self._handles[key] = self.predictor.make_batch(list(na), int(node_offset), int(graph_offset))
        return h

    @classmethod
    def from_config(cls, spec, device=None):
        """sample_cfg.classifier: a ClassifierGuidance, or a mapping {model_path, task, mode, target, scale, max_shift, start, stop,
        guide_types} whose predictor is read with predictor.load_predictor."""
        if spec is None or isinstance(spec, cls):
            return spec
        from .predictor import load_predictor
        d = {str(k): v for k, v in dict(spec).items()}
        if not d.get("model_path") or not d.get("task"):
            raise ValueError("sample_cfg.classifier needs model_path (a directory written by save_predictor) and task")
        unknown = set(d) - {"model_path", "task", "mode", "target", "scale", "max_shift", "start", "stop", "guide_types"}
        if unknown:
            raise ValueError(f"sample_cfg.classifier: unknown keys {sorted(unknown)}")
        pred = load_predictor(str(d.pop("model_path")), device=device)
        return cls(pred, **d)


def check_call(module, classifier, streams=None, record=False, noise=None, condition=None, likelihood=None, resample=None, guidance=None, steer=None):
    """sample(classifier=)'s refusals, by name, before any device work."""
    from .predictor import require_noised
    if not isinstance(classifier, ClassifierGuidance):
        raise ValueError(f"sample: classifier = takes a classifier.ClassifierGuidance, not {type(classifier).__name__}")
    if hasattr(module, "collate") or not hasattr(module, "beta_scheduler"):
        raise ValueError("sample(classifier=): the MatterGen-shaped module has no classifier-guided chain (DiffCSP only)")
    require_noised(classifier.predictor, "sample(classifier=)", module)
    if classifier.predictor.hparams.get("edge_style", "fc") != "fc":
        raise ValueError("sample(classifier=): a knn-style predictor has no input gradient (the fully connected pair mode only)")
    if streams is not None and int(streams) > 1:
        raise ValueError(f"sample(classifier=): streams = {streams}: a classifier-guided chain is one chain on one stream (streams = None means 1 here)")
    for name, v in (("record=True", record), ("noise", noise is not None), ("a condition", condition is not None), ("likelihood", likelihood is not None),
                    ("resample", resample is not None), ("guidance", guidance is not None), ("steer", steer is not None),
                    ("CSP mode", module.keep_lattice or module.keep_coords)):
        if v:
            raise ValueError(f"sample: classifier together with {name} is not supported")
    if getattr(module, "condition", None) is not None:
        raise ValueError("sample(classifier=): a property-conditioned prior is not classifier-guided (out of scope: guide the unconditional prior)")


def shift(classifier, handle, state, grads, coef):
    """One mi_guide_shift on the current stream: state = (frac_coords, lattices, atom_types), in place; grads = (g_frac, g_lat, g_types or
    None); coef = (a_t, a_x, a_l)."""
    from .cspnet import _ptr, _stream
    g_types = grads[2] if classifier.guide_types else None
    _lib.check(_lib.load().mi_guide_shift(handle._h, _ptr(state[2]), _ptr(state[0]), _ptr(state[1]), _ptr(g_types), _ptr(grads[0]), _ptr(grads[1]),
                                          coef[0], coef[1], coef[2], 0.0 if classifier.max_shift is None else classifier.max_shift, _stream()),
               "mi_guide_shift")


def run_chain(module, batch, classifier, step_lr, seed, init, t_start, t_stop, node_offset, graph_offset):
    """DiffCSPModule.sample(classifier=) after its checks: one chain on the current stream.  Returns (final, traj, info) with
    info = dict(levels, times, out [E][B] float32: the predictor's normalised output for the task at x_t of every guided step) -- host
    values from the call's one read, at its end."""
    from .cspnet import CrystalBatch, _ptr, _stream
    from .diffcsp import MAX_ATOMIC_NUM
    from .predictor import input_gradient
    lib = _lib.load()
    dev = module.device
    T = module.beta_scheduler.timesteps
    t_start = T if t_start is None else int(t_start)
    t_stop = int(t_stop)
    cb = batch if isinstance(batch, CrystalBatch) else module.crystal_batch(batch, node_offset, graph_offset)
    na = [int(v) for v in cb.num_atoms_list]
    B, N = cb.num_graphs, cb.num_nodes
    levels = classifier.window(t_start, t_stop)
    tau = module.time_map.tolist() if module.time_map is not None else None   # (a view: the predictor sees the trained time of the step index)
    times = [int(tau[k]) if tau is not None else int(k) for k in levels]
    ph = classifier.handle(na, node_offset, graph_offset)
    module.decoder.sync()
    if init is None:
        cur = (torch.empty(N, 3, device=dev), torch.empty(B, 3, 3, device=dev), torch.empty(N, MAX_ATOMIC_NUM, device=dev))
        _lib.check(lib.mi_sampler_init_state(cb._h, seed, T, _ptr(cur[2]), _ptr(cur[0]), _ptr(cur[1]), _stream()), "mi_sampler_init_state")
    else:
        cur = tuple(v.to(dev, torch.float32).contiguous().clone() for v in init)
    coef = module._coefficients(step_lr)
    coef_p = coef.numpy().ctypes.data_as(C.POINTER(C.c_float))
    _lib.check(lib.mi_sampler_set_keep(cb._h, 0, 0))
    E, P = len(levels), classifier.predictor.P
    bufs = dict(out=torch.empty(B, P, device=dev), d_out=torch.empty(B, P, device=dev), g_frac=torch.empty(N, 3, device=dev),
                g_lat=torch.empty(B, 3, 3, device=dev), g_types=torch.empty(N, MAX_ATOMIC_NUM, device=dev) if classifier.guide_types else None)
    book = torch.zeros(max(E, 1), B, device=dev)   # the predictor's output of every guided step, read once at the end

    def segment(a, b):
        _lib.check(lib.mi_sampler_run(module.decoder._h, cb._h, coef_p, T, a, b, _ptr(module.time_embedding.freqs), seed, None, None, _ptr(cur[2]),
                                      _ptr(cur[0]), _ptr(cur[1]), _stream()), "mi_sampler_run")

    at = t_start
    for e, (k, tk) in enumerate(zip(levels, times)):
        if k < at:   # the steps in front of the window: one ordinary, longer segment
            segment(at, k)
            at = k
        out, g_frac, g_lat, g_types = input_gradient(classifier.predictor, cur, ph, tk, task=classifier.task, mode=classifier.mode,
                                                     target=classifier.target, types=classifier.guide_types, bufs=bufs)
        book[e].copy_(out[:, classifier.p])
        segment(k, k - 1)
        at = k - 1
        shift(classifier, ph, cur, (g_frac, g_lat, g_types), classifier.coefficients(module, step_lr, k))
    if at > t_stop:
        segment(at, t_stop)
    if cb.edge_style == "knn":
        module.__dict__.setdefault("_knn_pending", []).append((cb, torch.cuda.current_stream()))
    x, l, a = cur
    final = dict(atom_types=a, frac_coords=x, lattices=l, num_atoms=cb.num_atoms, batch_idx=cb.batch)
    host = book.cpu()   # the one read
    info = dict(levels=list(levels), times=times, out=host[:E].clone())
    return final, {t_stop: final}, info
