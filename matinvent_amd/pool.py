"""A device-memory pool for batch handles (include/matinvent_hip_pool.h).

pretrain.fit's mini-batches each have their own atom counts, so each creates a batch handle, runs one micro-step on it and releases it.
A handle created in a HandlePool keeps its exact-size buffers, but the memory behind them outlives it: the next handle takes the blocks
over, in stream order, and neither the creation nor the release waits for the device.

    pool = HandlePool()
    cb = model.make_batch(num_atoms, pool=pool)      # or CrystalBatch(net, num_atoms, pool=pool)
    ...
    cb.release()                                     # the blocks go back to the pool; nothing is freed
    pool.close()                                     # frees everything (every handle must have been released)

A pool belongs to ONE stream (the current stream when it is created, unless `stream` is given) and its handles are used on that stream
only; the library checks that.  The sampler, the RL steps and every entry that attaches state to a handle refuse a pooled handle.
"""
import ctypes as C

import torch

from . import _lib

STATS = ("bytes_reserved", "bytes_in_use", "mallocs", "reuses", "frees", "live_handles", "bytes_high_water", "max_bytes")


def parse_handle_pool(value):
    """cfg.handle_pool -> None (no pool) or the keyword arguments of HandlePool: false / None (the default), true, or a mapping
    {max_bytes: int or None}.  Anything else is a ValueError."""
    if value is None or value is False:
        return None
    if value is True:
        return {}
    if isinstance(value, (str, bytes, int, float)) or not (hasattr(value, "keys") and hasattr(value, "__getitem__")):
        raise ValueError(f"handle_pool = {value!r}: it takes false, true or {{max_bytes: ...}}")
    spec = {k: value[k] for k in value.keys()}
    extra = set(spec) - {"max_bytes"}
    if extra:
        raise ValueError(f"handle_pool: unknown key(s) {sorted(extra)}; it takes max_bytes")
    mb = spec.get("max_bytes")
    if mb is None:
        return {}
    if isinstance(mb, bool) or not isinstance(mb, int) or mb <= 0:
        raise ValueError(f"handle_pool.max_bytes = {mb!r}: a positive number of bytes (or null for no cap)")
    return {"max_bytes": int(mb)}


def block_bytes(request: int) -> int:
    """The pool's size class of a request of `request` bytes (mi_pool_block_bytes; host only)."""
    return int(_lib.load().mi_pool_block_bytes(int(request)))


class HandlePool:
    """mi_pool: the memory behind pooled batch handles of one stream.  max_bytes=None: no cap; with a cap, a handle that does not fit
    even after the cached blocks were freed raises MIError (MI_ENOMEM) and leaves the pool usable.  poison=True (a debug aid) fills every
    float / fp16 block with quiet NaN before it is handed out."""

    def __init__(self, max_bytes=None, poison=False, stream=None):
        lib = _lib.load()
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else 0
        elif hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        h = C.c_void_p()
        self._h = None
        self._lib = lib
        _lib.check(lib.mi_pool_create(C.c_void_p(int(stream)), int(max_bytes or 0), C.byref(h)), "mi_pool_create")
        self._h = h
        self.stream = int(stream)
        if poison:
            _lib.check(lib.mi_pool_set_poison(h, 1), "mi_pool_set_poison")

    def _handle(self):
        if self._h is None:
            raise RuntimeError("HandlePool: the pool is closed")
        return self._h

    def stats(self) -> dict:
        out = (C.c_int64 * 8)()
        _lib.check(self._lib.mi_pool_stats(self._handle(), out), "mi_pool_stats")
        return dict(zip(STATS, (int(v) for v in out)))

    def trim(self):
        """Free every cached block that no handle holds (waits for the pool's stream)."""
        _lib.check(self._lib.mi_pool_trim(self._handle()), "mi_pool_trim")

    def close(self):
        """Free everything; MIError (MI_ESTATE) while a handle created in the pool is alive -- the pool stays open then."""
        h = getattr(self, "_h", None)
        if h is not None:
            _lib.check(self._lib.mi_pool_destroy(h), "mi_pool_destroy")
            self._h = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and getattr(self, "_lib", None) is not None:
            self._lib.mi_pool_destroy(h)   # (live handles: the pool is left alone -- their release must still find it)
