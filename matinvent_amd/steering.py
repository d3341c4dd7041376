"""Predictor-steered sampling: particle resampling along the reverse chain (include/matinvent_hip_steer.h).

Feynman-Kac steering (sequential Monte Carlo with twisted resampling): the chain runs K particles per crystal; at chosen noise levels a
NOISE-AWARE property predictor (predictor.fit_predictor(diffusion=)) scores every particle's noisy state, and the particles of each group
are resampled in proportion to exp(scale * (u - u_prev)).  The difference potentials telescope: the particle system targets
p_prior(x_0) exp(scale * u(x_0)) -- the distribution the KL-anchored RL loops move the weights towards -- without a training step, an
input gradient, or a change to any kernel of the chain.

The chain is walked as segments of mi_sampler_run between the steering levels; at a level the predictor's forward on the state
(mi_scalar_forward_state, on a handle of the predictor's own) and mi_steer_resample into the other of two state buffers, which then
swap.  Everything is enqueued on the current stream; the host reads nothing until the chain has ended.  `scale` is untuned."""
import ctypes as C

import numpy as np
import torch

from . import _lib

MODES = {"max": _lib.STEER_MODE_MAX, "min": _lib.STEER_MODE_MIN, "target": _lib.STEER_MODE_TARGET}
STATS = ("resampled_groups", "ess_sum", "groups_without_finite_weight")   # mi_steer_resample's stats[0..2]


def refuse(where, **keys):
    """A resampled particle system has no per-chain trajectory likelihood: sample_mdp / sample_rollout / MatInventPG refuse the steering key."""
    for k, v in keys.items():
        if v is not None:
            raise ValueError(f"{where}: {k} is not supported -- a steered chain is a resampled particle system, which has no per-chain "
                             "trajectory likelihood (DESIGN 43)")


class Steering:
    """What a steered chain needs besides the prior.  predictor: a noise-aware PropertyPredictor; task: one of its property names;
    mode: "max" / "min" / "target" (then target = the raw property value aimed at); particles = K replicas per crystal (1..256);
    scale = lambda, the inverse temperature of the tilt in the predictor's NORMALISED units (untuned); every = m: an event every m steps
    counted down from the chain's start -- or levels = [...]: the explicit step indices; ess = None: resample at every event, or tau in
    (0, 1]: only the groups whose effective sample size has fallen below tau K."""

    def __init__(self, predictor, task, mode="max", target=None, particles=4, scale=1.0, every=None, levels=None, ess=None):
        from .predictor import require_noised
        require_noised(predictor, "Steering")
        if task not in predictor.names:
            raise ValueError(f"Steering: task = {task!r} is not a property of the predictor ({predictor.names})")
        if mode not in MODES:
            raise ValueError(f"Steering: mode = {mode!r}: it takes 'max', 'min' or 'target'")
        if (mode == "target") != (target is not None):
            raise ValueError("Steering: target = goes with mode = 'target', and only with it")
        if target is not None and not np.isfinite(float(target)):
            raise ValueError(f"Steering: target = {target} is not finite")
        K = int(particles)
        if not 1 <= K <= _lib.STEER_MAX_PARTICLES:
            raise ValueError(f"Steering: particles = {particles}: 1..{_lib.STEER_MAX_PARTICLES}")
        if not np.isfinite(float(scale)):
            raise ValueError(f"Steering: scale = {scale} is not finite")
        if (every is None) == (levels is None):
            raise ValueError("Steering: give every = m or levels = [...], exactly one of the two")
        if every is not None and int(every) < 1:
            raise ValueError(f"Steering: every = {every}: must be >= 1")
        if levels is not None:
            levels = sorted({int(v) for v in levels}, reverse=True)
            if not levels or levels[-1] < 0:
                raise ValueError("Steering: levels = needs at least one step index, none negative")
        if ess is not None and not 0.0 < float(ess) <= 1.0:
            raise ValueError(f"Steering: ess = {ess}: None (always resample) or a fraction in (0, 1]")
        self.predictor, self.task, self.mode = predictor, str(task), mode
        self.p = predictor.names.index(task)
        self.target = None if target is None else float(target)
        self.particles, self.scale = K, float(scale)
        self.every = None if every is None else int(every)
        self.levels = levels
        self.ess = None if ess is None else float(ess)
        self._handles = {}

    @property
    def target_hat(self):
        """The target in the predictor's normalised units (0 when the mode takes none)."""
        if self.target is None:
            return 0.0
        nm = self.predictor.normalizer
        return (self.target - float(nm.mean[self.p])) / float(nm.std[self.p])

    @property
    def ess_frac(self):
        return -1.0 if self.ess is None else self.ess

    def replicate(self, num_atoms):
        """The G K atom counts of a steered batch: every crystal's count K times in a row (the groups mi_steer_resample reads)."""
        na = num_atoms.tolist() if hasattr(num_atoms, "tolist") else list(num_atoms)
        return [int(v) for v in na for _ in range(self.particles)]

    def check_counts(self, num_atoms, where="sample(steer=)"):
        na = [int(v) for v in (num_atoms.tolist() if hasattr(num_atoms, "tolist") else num_atoms)]
        K = self.particles
        if len(na) % K != 0 or any(na[c] != na[(c // K) * K] for c in range(len(na))):
            raise ValueError(f"{where}: the atom counts are not K-replicated (groups of K = {K} consecutive crystals of one atom count: "
                             "Steering.replicate(num_atoms) builds them)")
        return na

    def schedule(self, t_start, t_stop=0):
        """The step indices of the events of a chain from t_start down to t_stop, descending: with every = m the levels k < t_start with
        (t_start - k) % m == 0 down to t_stop itself (the last event sits on the final state when m divides the chain's length); with
        levels = [...] those of them in t_stop .. t_start - 1.  On a respaced view these are indices of the view's own grid."""
        t_start, t_stop = int(t_start), int(t_stop)
        if self.every is not None:
            return list(range(t_start - self.every, t_stop - 1, -self.every))
        return [k for k in self.levels if t_stop <= k < t_start]

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
        """sample_cfg.steer: a Steering, or a mapping {model_path, task, mode, target, particles, scale, every | levels, ess} whose
        predictor is read with predictor.load_predictor."""
        if spec is None or isinstance(spec, cls):
            return spec
        from .predictor import load_predictor
        d = {str(k): v for k, v in dict(spec).items()}
        if not d.get("model_path") or not d.get("task"):
            raise ValueError("sample_cfg.steer needs model_path (a directory written by save_predictor) and task")
        pred = load_predictor(str(d.pop("model_path")), device=device)
        unknown = set(d) - {"task", "mode", "target", "particles", "scale", "every", "levels", "ess"}
        if unknown:
            raise ValueError(f"sample_cfg.steer: unknown keys {sorted(unknown)}")
        if d.get("levels") is not None:
            d["levels"] = [int(v) for v in d["levels"]]
        return cls(pred, **d)


def check_call(module, steer, streams=None, record=False, noise=None, condition=None, likelihood=None, resample=None, guidance=None):
    """sample(steer=)'s refusals, by name, before any device work."""
    from .predictor import require_noised
    if not isinstance(steer, Steering):
        raise ValueError(f"sample: steer = takes a steering.Steering, not {type(steer).__name__}")
    if hasattr(module, "collate") or not hasattr(module, "beta_scheduler"):
        raise ValueError("sample(steer=): the MatterGen-shaped module has no steered chain (DiffCSP only)")
    require_noised(steer.predictor, "sample(steer=)", module)
    if streams is not None and int(streams) > 1:
        raise ValueError(f"sample(steer=): streams = {streams}: a steered chain is one chain on one stream (streams = None means 1 here)")
    for name, v in (("record=True", record), ("noise", noise is not None), ("a condition", condition is not None), ("likelihood", likelihood is not None),
                    ("resample", resample is not None), ("guidance", guidance is not None),
                    ("CSP mode", module.keep_lattice or module.keep_coords)):
        if v:
            raise ValueError(f"sample: steer together with {name} is not supported")
    if getattr(module, "condition", None) is not None:
        raise ValueError("sample(steer=): a property-conditioned prior is not steered (out of scope: steer the unconditional prior)")


def resample(steer, handle, out, level, seed, u_prev, logw, src, dst, ancestors, stats):
    """One mi_steer_resample on the current stream: src / dst = (frac_coords, lattices, atom_types) state tuples, two different buffers."""
    from .cspnet import _ptr, _stream
    _lib.check(_lib.load().mi_steer_resample(handle._h, steer.particles, _ptr(out), steer.predictor.P, steer.p, MODES[steer.mode], steer.target_hat,
                                             steer.scale, steer.ess_frac, int(seed), int(level) & 0xFFFFFFFF, _ptr(u_prev), _ptr(logw), _ptr(src[2]),
                                             _ptr(src[0]), _ptr(src[1]), _ptr(dst[2]), _ptr(dst[0]), _ptr(dst[1]), _ptr(ancestors), _ptr(stats),
                                             _stream()), "mi_steer_resample")


def run_chain(module, batch, steer, step_lr, seed, init, t_start, t_stop, node_offset, graph_offset):
    """DiffCSPModule.sample(steer=) after its checks: one chain on the current stream.  Returns (final, traj, info) with
    info = dict(levels, times, ancestors [E][B] int32, stats [E][3] float32) -- host tensors from the call's one read, at its end."""
    from .cspnet import CrystalBatch, _ptr, _stream
    from .diffcsp import MAX_ATOMIC_NUM
    from .predictor import forward_state
    lib = _lib.load()
    dev = module.device
    T = module.beta_scheduler.timesteps
    t_start = T if t_start is None else int(t_start)
    cb = batch if isinstance(batch, CrystalBatch) else module.crystal_batch(batch, node_offset, graph_offset)
    na = steer.check_counts(cb.num_atoms_list)
    B, N = cb.num_graphs, cb.num_nodes
    levels = steer.schedule(t_start, t_stop)
    tau = module.time_map.tolist() if module.time_map is not None else None   # (a view: the predictor sees the trained time of the step index)
    times = [int(tau[k]) if tau is not None else int(k) for k in levels]
    ph = steer.handle(na, node_offset, graph_offset)
    module.decoder.sync()
    if init is None:
        cur = (torch.empty(N, 3, device=dev), torch.empty(B, 3, 3, device=dev), torch.empty(N, MAX_ATOMIC_NUM, device=dev))
        _lib.check(lib.mi_sampler_init_state(cb._h, seed, T, _ptr(cur[2]), _ptr(cur[0]), _ptr(cur[1]), _stream()), "mi_sampler_init_state")
    else:
        cur = tuple(v.to(dev, torch.float32).contiguous().clone() for v in init)
    other = tuple(torch.empty_like(v) for v in cur)
    coef = module._coefficients(step_lr)
    coef_p = coef.numpy().ctypes.data_as(C.POINTER(C.c_float))
    _lib.check(lib.mi_sampler_set_keep(cb._h, 0, 0))
    E = len(levels)
    P = steer.predictor.P
    out = torch.empty(B, P, device=dev)
    u_prev, logw = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    # ancestors and statistics of every event in ONE buffer (row e: B ints, then 3 floats), read once at the end
    book = torch.zeros(max(E, 1), B + _lib.STEER_NSTATS, dtype=torch.int32, device=dev)

    def segment(state, a, b):
        _lib.check(lib.mi_sampler_run(module.decoder._h, cb._h, coef_p, T, a, b, _ptr(module.time_embedding.freqs), seed, None, None, _ptr(state[2]),
                                      _ptr(state[0]), _ptr(state[1]), _stream()), "mi_sampler_run")

    at = t_start
    for e, (k, tk) in enumerate(zip(levels, times)):
        if k < at:
            segment(cur, at, k)
            at = k
        forward_state(steer.predictor, cur, ph, tk, out=out)
        resample(steer, ph, out, k, seed, u_prev, logw, cur, other, book[e, :B], book[e, B:].view(torch.float32))
        cur, other = other, cur
    if at > t_stop:
        segment(cur, at, t_stop)
    if cb.edge_style == "knn":
        module.__dict__.setdefault("_knn_pending", []).append((cb, torch.cuda.current_stream()))
    x, l, a = cur
    final = dict(atom_types=a, frac_coords=x, lattices=l, num_atoms=cb.num_atoms, batch_idx=cb.batch)
    host = book.cpu()   # the one read
    info = dict(levels=list(levels), times=times, ancestors=host[:E, :B].clone(), stats=host[:E, B:].clone().view(torch.float32))
    return final, {t_stop: final}, info
