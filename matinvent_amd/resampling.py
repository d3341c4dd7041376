"""Resampling jumps for the conditioned reverse chain (include/matinvent_hip_resample.h): RePaint's "time travel" (Lugmayr et
al. 2022).  Replacement conditioning (conditioning.py) overwrites the known part after every reverse step with a forward-noised copy that
is drawn independently of what the chain generated; with resample=(r, j) the chain re-noises the WHOLE state j levels forward at every
jump-off level 1, 1 + j, 1 + 2 j, ... and denoises again, r visits in all, so the generated part gets several passes at adapting to the
imposed part.  Host bookkeeping only: the jump table, the schedule, the per-visit seeds; the jump is resample_jump_kernel
(csrc/resample.hip) and the chain is mi_sampler_run's."""
import ctypes as C

import numpy as np
import torch

DRAW_JUMP_L, DRAW_JUMP_X, DRAW_JUMP_T, DRAW_VISIT = 24, 25, 26, 27


def jump_table(module, j, dtype=torch.float32) -> torch.Tensor:
    """[T + 1, 3]: row a = (c0, c1, s) of the forward jump a -> b = a + j, c0 = sqrt(abar_b / abar_a), c1 = sqrt(1 - abar_b / abar_a),
    s = sqrt(sigma_b^2 - sigma_a^2); rows with a + j > T are zero.  Computed in float64 from the module's own schedulers (on a strided view
    the view's tables, so the level is the step index there too) and rounded to `dtype` at the end: in float32 1 - c0^2 cancels at the
    early levels, where abar_b / abar_a is within a few ulp of 1."""
    ac = module.beta_scheduler.alphas_cumprod.detach().cpu().double()
    sig = module.sigma_scheduler.sigmas.detach().cpu().double()
    n, j = len(ac), int(j)
    if j < 1 or j >= n:
        raise ValueError(f"jump_table: the jump length must lie in 1..{n - 1} (got {j})")
    tab = torch.zeros(n, 3, dtype=torch.float64)
    ratio = ac[j:] / ac[:n - j]
    tab[:n - j, 0] = torch.sqrt(ratio)
    tab[:n - j, 1] = torch.sqrt((1.0 - ratio).clamp_min(0.0))
    tab[:n - j, 2] = torch.sqrt((sig[j:] ** 2 - sig[:n - j] ** 2).clamp_min(0.0))
    return tab.to(dtype).contiguous()


def check(where, resample):
    """The `resample` keyword: None, or (r, j) with r >= 1 visits per jump-off level and jumps of j >= 1 levels.  Returns (r, j) or None."""
    if resample is None:
        return None
    try:
        r, j = resample
        ok = int(r) == r and int(j) == j
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{where}: resample = {resample!r} is not a pair of integers (r, j)")
    r, j = int(r), int(j)
    if r < 1 or j < 1:
        raise ValueError(f"{where}: resample = (r, j) = ({r}, {j}) needs r >= 1 and j >= 1")
    return r, j


def schedule(t_start, r, j) -> list:
    """The levels a chain with resampling (r, j) started at t_start visits, t_start first and 0 last (mi_resample_schedule's list)."""
    t_start, r, j = int(t_start), int(r), int(j)
    if t_start < 0 or r < 1 or j < 1:
        raise ValueError(f"schedule: t_start = {t_start}, r = {r}, j = {j} (t_start >= 0, r >= 1, j >= 1)")
    left = {L: r - 1 for L in range(1, t_start - j + 1, j)}
    t, levels = t_start, [t_start]
    while t > 0:
        t -= 1
        levels.append(t)
        if left.get(t, 0) > 0:
            left[t] -= 1
            t += j
            levels.append(t)
    return levels


def walk(t_start, r, j, seed):
    """The chain's moves in order: ("step", t, seed_v) for the reverse step t -> t - 1 (and the imposition at t - 1 that follows it), v its
    0-based repetition; ("jump", a, seed_v) for the forward jump a -> a + j, v the 1-based count of jumps off level a."""
    levels = schedule(t_start, r, j)
    steps, jumps, out = {}, {}, []
    for a, b in zip(levels[:-1], levels[1:]):
        if b == a - 1:
            out.append(("step", a, visit_seed(seed, steps.get(a, 0))))
            steps[a] = steps.get(a, 0) + 1
        else:
            jumps[a] = jumps.get(a, 0) + 1
            out.append(("jump", a, visit_seed(seed, jumps[a])))
    return out


_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def visit_seed(seed, v) -> int:
    """seed_v: seed_0 = seed; for v >= 1 words 0 (low) and 1 (high) of the Philox4x32-10 block with counter (0, 0, DRAW_VISIT, v) under
    the key `seed` (mi_resample_visit_seed)."""
    seed, v = int(seed) & 0xFFFFFFFFFFFFFFFF, int(v)
    if not 0 <= v <= _MASK:
        raise ValueError(f"visit_seed: v = {v} outside 0..2^32 - 1")
    if v == 0:
        return seed
    c, k0, k1 = [0, 0, DRAW_VISIT, v], seed & _MASK, seed >> 32
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & _MASK, (p0 >> 32) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c[0] | (c[1] << 32)


def check_chain(where, resample, T, t_start=None, t_stop=0, condition=None, record=False, noise=None, likelihood=None):
    """What a resampled chain needs (ValueError before any device work): a condition; no record, no teacher-forced noise, no likelihood
    keyword; t_stop = 0; and with r > 1 at least one jump-off level (1 + j <= t_start).  Returns (r, j) or None."""
    rj = check(where, resample)
    if rj is None:
        return None
    r, j = rj
    if condition is None:
        raise ValueError(f"{where}: resample needs a condition -- the jumps let the generated part adapt to the imposed part")
    if record:
        raise ValueError(f"{where}: resample with record=True is not supported -- a resampled chain visits levels more than once")
    if noise is not None:
        raise ValueError(f"{where}: resample with teacher-forced noise is not supported -- `noise` holds one draw per level")
    if likelihood is not None:
        raise ValueError(f"{where}: resample with likelihood = {likelihood!r} is not supported -- a resampled chain records no likelihood")
    if int(t_stop) != 0:
        raise ValueError(f"{where}: resample needs t_stop = 0 (got {t_stop})")
    t_start = int(T if t_start is None else t_start)
    if j >= T + 1 or 1 + j > t_start:
        raise ValueError(f"{where}: resample = ({r}, {j}) has no jump-off level on a chain started at {t_start} (1 + j <= t_start)")
    return rj


def refuse(where, **keys):
    """The trajectory layer models one visit per level: sample_mdp / sample_rollout / MatInventPG refuse the resampling keys."""
    for k, v in keys.items():
        if v is not None:
            raise ValueError(f"{where}: {k} = {v!r} is not supported -- a resampled chain visits levels more than once, and the trajectory "
                             "layer models one visit (DESIGN 37)")


def attach(module, cb, r, j, table=None):
    """Copy (r, j) and `module`'s jump table to the batch handle `cb` (mi_batch_set_resampling: a blocking copy; no work of the handle may
    be in flight).  `table`: a [n, 3] table instead of the module's (tests)."""
    from . import _lib
    tab = (jump_table(module, j) if table is None else torch.as_tensor(table).float()).contiguous().numpy()
    _lib.check(_lib.load().mi_batch_set_resampling(cb._h, tab.ctypes.data_as(C.POINTER(C.c_float)), int(tab.shape[0]), int(r), int(j)),
               "mi_batch_set_resampling")


def clear(cb):
    from . import _lib
    _lib.check(_lib.load().mi_batch_set_resampling(cb._h, None, 0, 1, 0), "mi_batch_set_resampling")


def jump(cb, from_level, seed, atom_types, frac_coords, lattices):
    """mi_resample_jump: the forward jump from_level -> from_level + j of a state (device tensors, float32, contiguous; in place) under the
    resampling attached to `cb`, on the current stream."""
    from . import _lib
    from .cspnet import _ptr, _stream
    for v in (atom_types, frac_coords, lattices):
        assert v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()
    _lib.check(_lib.load().mi_resample_jump(cb._h, int(from_level), int(seed), _ptr(atom_types), _ptr(frac_coords), _ptr(lattices), _stream()),
               "mi_resample_jump")


def library_schedule(t_start, r, j) -> list:
    """mi_resample_schedule's list: the definition the chain's driver reads."""
    from . import _lib
    lib = _lib.load()
    n = int(lib.mi_resample_schedule(int(t_start), int(r), int(j), None, 0))
    if n < 0:
        _lib.check(n, "mi_resample_schedule")
    buf = np.zeros(n, dtype=np.int32)
    got = int(lib.mi_resample_schedule(int(t_start), int(r), int(j), buf.ctypes.data_as(C.POINTER(C.c_int)), n))
    assert got == n
    return buf.tolist()
