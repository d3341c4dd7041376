"""A property-conditioned DiffCSP prior and classifier-free guidance: the host side of include/matinvent_hip_guidance.h.

A crystal carries P >= 1 scalar properties.  They are normalised here in float64, y^ = (y - mu) / sigma (PropertyNormalizer), and cross to
the device as float32 `yhat` [B][P] with an int32 `have` [B][P]: a missing value -- absent, None or NaN -- is have = 0, never a NaN on the
device.  The network reads them as 2 F columns per property, sin / cos of w_k clamp(y^, -8, 8) with w_k = (pi / 8) 2^k (property_freqs),
behind the time embedding; the NULL condition (a missing value, a dropped crystal, no values at all) is 2 F exact zeros.

Training drops a crystal's condition with probability p_uncond, drawn on the device from the Philox stream of the micro-step at draw id
28, indexed by the crystal's position in the whole mini-batch (drop_mask restates the draw on the host).  Sampling under
Guidance(values, factor) evaluates the network twice per stage and steps with p_c + factor (p_c - p_u).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

MAX_FREQS, CLAMP = _lib.GUIDANCE_MAX_FREQS, _lib.GUIDANCE_CLAMP
DRAW_COND_DROP = 28   # csrc/common.h


def property_freqs(F):
    """float32 [F]: w_k = (pi / 8) 2^k -- the largest period spans the clamp range [-8, 8] twice over, every further one halves it."""
    F = int(F)
    if not 1 <= F <= MAX_FREQS:
        raise ValueError(f"property_freqs: num_freqs = {F} lies outside 1..{MAX_FREQS}")
    return torch.from_numpy((math.pi / 8.0 * 2.0 ** np.arange(F)).astype(np.float32))


def latent_dim(P, F):
    """Z = 2 F P: the columns the property part adds to the embedding (DiffCSPModule(latent_dim=Z))."""
    return 2 * int(F) * int(P)


def _missing(v):
    if v is None:
        return True
    try:
        return not math.isfinite(float(v))
    except (TypeError, ValueError):
        return True


class PropertyNormalizer:
    """Names, mean and standard deviation per property.  fit() ignores missing values (a property nobody has: mean 0, std 1); a
    standard deviation of 0 becomes 1."""

    def __init__(self, names, mean=None, std=None):
        self.names = [str(n) for n in names]
        if not self.names or len(set(self.names)) != len(self.names):
            raise ValueError(f"PropertyNormalizer: the property names {self.names} must be distinct and at least one")
        P = len(self.names)
        self.mean = np.zeros(P) if mean is None else np.asarray(mean, dtype=np.float64).reshape(P)
        self.std = np.ones(P) if std is None else np.asarray(std, dtype=np.float64).reshape(P)
        self.std = np.where(self.std == 0, 1.0, self.std)

    @property
    def P(self):
        return len(self.names)

    def raw(self, items):
        """float64 [n][P] of the records' values (CrystalData.properties, or dicts), NaN where missing."""
        out = np.full((len(items), self.P), np.nan)
        for i, d in enumerate(items):
            props = d if isinstance(d, dict) else (getattr(d, "properties", None) or {})
            for p, name in enumerate(self.names):
                v = props.get(name)
                if not _missing(v):
                    out[i, p] = float(v)
        return out

    def fit(self, items):
        y = self.raw(items)
        for p in range(self.P):
            v = y[~np.isnan(y[:, p]), p]
            self.mean[p] = v.mean() if v.size else 0.0
            s = v.std() if v.size else 1.0
            self.std[p] = s if s > 0 else 1.0
        return self

    def normalise(self, y):
        """(yhat float32 [n][P], have int32 [n][P]) of raw values [n][P] (NaN: missing; yhat is 0 there)."""
        y = np.asarray(y, dtype=np.float64).reshape(-1, self.P)
        have = np.isfinite(y)
        yhat = np.where(have, (np.where(have, y, 0.0) - self.mean) / self.std, 0.0)
        return np.ascontiguousarray(yhat, dtype=np.float32), np.ascontiguousarray(have, dtype=np.int32)

    def __call__(self, items):
        return self.normalise(self.raw(items))

    def to_dict(self):
        return dict(properties=list(self.names), mean=[float(v) for v in self.mean], std=[float(v) for v in self.std])


def parse_condition(spec):
    """cfg.condition = {properties: [...], num_freqs: F, p_uncond: 0.1} -> dict(properties, num_freqs, p_uncond), or None.  ValueError for
    an unknown key, no property, num_freqs outside 1..12 or p_uncond outside [0, 1]."""
    if spec is None:
        return None
    spec = {k: spec[k] for k in spec}
    extra = set(spec) - {"properties", "num_freqs", "p_uncond", "mean", "std"}
    if extra:
        raise ValueError(f"condition: unknown key(s) {sorted(extra)}; it takes properties, num_freqs, p_uncond")
    names = spec.get("properties")
    names = [names] if isinstance(names, str) else [str(n) for n in (names or [])]
    if not names or len(set(names)) != len(names):
        raise ValueError("condition: `properties` must list at least one property name, each once")
    F = int(spec.get("num_freqs", 8))
    if not 1 <= F <= MAX_FREQS:
        raise ValueError(f"condition: num_freqs = {F} lies outside 1..{MAX_FREQS}")
    p = float(spec.get("p_uncond", 0.1))
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"condition: p_uncond = {p} lies outside [0, 1]")
    out = dict(properties=names, num_freqs=F, p_uncond=p)
    for k in ("mean", "std"):
        if spec.get(k) is not None:
            v = [float(x) for x in spec[k]]
            if len(v) != len(names):
                raise ValueError(f"condition: {k} holds {len(v)} values for {len(names)} properties")
            out[k] = v
    return out


def module_condition(model, where):
    """The parsed condition of a module with a property part (hparams["condition"]), or ValueError by `where`'s name."""
    cond = getattr(model, "condition", None)
    if cond is None:
        raise ValueError(f"{where}: the module has no property part (DiffCSPModule(latent_dim=2 F P, condition={{properties, num_freqs}}))")
    return cond


def refuse_latent(model, where):
    """ValueError by name, before any device work: the entries behind `where` fill the time embedding alone (RL on a conditional prior is
    a follow-up)."""
    for m in (model,) if not isinstance(model, (tuple, list)) else model:
        if m is not None and getattr(m, "condition", None) is not None:
            raise ValueError(f"{where}: a property-conditioned prior (latent_dim > 0) is not taken here -- reinforcement learning and "
                             "trajectory likelihoods on a conditional prior are not built yet; pretrain.fit trains it, sample(guidance=) samples it")


# ---- the dropout draw on the host ------------------------------------------------------------------------------------------------

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def _philox4x32_10(c, k0, k1):
    """Philox4x32-10 over counters c [n][4] (uint64 arrays holding 32-bit words) under the key (k0, k1): csrc/common.h's rounds."""
    c0, c1, c2, c3 = (c[:, i].astype(np.uint64) for i in range(4))
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n1 = p1 & mask
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        n3 = p0 & mask
        c0, c1, c2, c3 = n0 & mask, n1, n2 & mask, n3
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1)


def drop_uniforms(seed, call_id, B, graph_offset=0):
    """float32 [B]: the uniforms in [0, 1) of draw id 28 at call `call_id` for the crystals graph_offset .. graph_offset + B - 1 of the
    mini-batch (element e: word e & 3 of the block at counter (e >> 2, 28, call_id))."""
    e = np.arange(int(graph_offset), int(graph_offset) + int(B), dtype=np.uint64)
    quad = e >> np.uint64(2)
    ctr = np.stack([quad & np.uint64(0xFFFFFFFF), quad >> np.uint64(32), np.full_like(quad, DRAW_COND_DROP),
                    np.full_like(quad, int(call_id) & 0xFFFFFFFF)], axis=1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    words = _philox4x32_10(ctr, seed & 0xFFFFFFFF, seed >> 32)
    w = words[np.arange(len(e)), (e & np.uint64(3)).astype(np.int64)]
    return ((w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def drop_mask(seed, call_id, B, p_uncond, graph_offset=0):
    """bool [B]: the crystals the micro-step at (seed, call_id) leaves without a condition -- uniform < float32(p_uncond); p_uncond = 0
    drops none (and the device makes no draw)."""
    if float(p_uncond) <= 0.0:
        return np.zeros(int(B), dtype=bool)
    return drop_uniforms(seed, call_id, B, graph_offset) < np.float32(p_uncond)


# ---- sampling ---------------------------------------------------------------------------------------------------------------------

class Guidance:
    """What a guided chain is conditioned on: values = {"density": 5.0} (every crystal) or {"density": array [B]} (per crystal; NaN:
    that crystal has none), and the guidance factor gamma -- 0: the conditional chain, one evaluation per stage; gamma != 0: two, stepping
    with p_c + gamma (p_c - p_u)."""

    def __init__(self, values, factor=0.0):
        if not isinstance(values, dict) or not values:
            raise ValueError("Guidance: `values` is a non-empty dict name -> value or per-crystal array")
        self.values = dict(values)
        self.factor = float(factor)
        if not math.isfinite(self.factor):
            raise ValueError(f"Guidance: factor = {factor} is not finite")

    def arrays(self, normalizer, B):
        """(yhat float32 [B][P], have int32 [B][P]) under `normalizer`.  ValueError: a name the normaliser does not know, an array of
        another length than B."""
        unknown = sorted(set(self.values) - set(normalizer.names))
        if unknown:
            raise ValueError(f"Guidance: the model was not trained on {unknown}; it knows {normalizer.names}")
        y = np.full((int(B), normalizer.P), np.nan)
        for name, v in self.values.items():
            a = np.asarray(v.cpu() if torch.is_tensor(v) else v, dtype=np.float64)
            if a.ndim == 0:
                a = np.full(int(B), float(a))
            a = a.reshape(-1)
            if a.shape[0] != int(B):
                raise ValueError(f"Guidance: {name} holds {a.shape[0]} values for {int(B)} crystals")
            y[:, normalizer.names.index(name)] = a
        return normalizer.normalise(y)


def attach(cb, partner, yhat, have, F, factor):
    """mi_batch_set_guidance on the handle `cb` (blocking copies: no work of the handle in flight)."""
    P = yhat.shape[1]
    _lib.check(_lib.load().mi_batch_set_guidance(cb._h, None if partner is None else partner._h, yhat.ctypes.data_as(C.POINTER(C.c_float)),
                                                 have.ctypes.data_as(C.POINTER(C.c_int)), int(P), int(F), float(factor)), "mi_batch_set_guidance")


def clear(cb):
    _lib.check(_lib.load().mi_batch_clear_guidance(cb._h), "mi_batch_clear_guidance")
