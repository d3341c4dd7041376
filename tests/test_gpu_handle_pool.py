"""GPU checks of pooled batch handles (include/matinvent_hip_pool.h; matinvent_amd/csrc/pool.hip; matinvent_amd/pool.py).

A pooled handle has the layout of a classic one, so every comparison here is EXACT: np.array_equal index tables, torch.equal statistics,
per-crystal sums, predictions and gradients against a classic handle that is given the same times, seed, Philox call id and device noise.
The pools run with poison on unless a test is about something else: a float or fp16 block is quiet NaN when it is handed out, so a buffer
that relied on fresh pages being zero would show as NaN.  64-wide, 2-layer network, T = 1000, unless the test says otherwise.

(1) tables  (2) recycled, poisoned memory gives the same bits  (3) the same at the tape's plane-set branch  (4) inference and
forward-only  (5) no allocation after warm-up  (6) the cap  (7) fit  (8) refusals."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from matinvent_amd import _lib
from oracle import diffcsp_oracle as O
from tests import ft_ref64 as R
from tests.gpu_util import make_module

pytestmark = pytest.mark.gpu

T = 1000
SEED = 1234
MIX = [1, 7, 20, 3, 13]
TABLES = ("num_atoms", "node2graph", "rowptr", "e_diag", "src", "dst", "edge_graph", "pair_i", "pair_j", "pair_e1", "pair_e2", "pair_graph",
          "node_off", "pair_off")


def _pool(**kw):
    from matinvent_amd.pool import HandlePool
    return HandlePool(**kw)


def _params(H, seed=5):
    P = O.init_params(O.CSPNetHParams(hidden_dim=H, num_layers=2, num_freqs=8), seed=seed)
    gen = torch.Generator().manual_seed(seed + 100)
    for k in P:
        if "layer_norm" in k:
            P[k] = P[k] + 0.1 * torch.randn(P[k].shape, generator=gen)
    return P


@functools.lru_cache(maxsize=None)
def _module(H=64):
    sn = torch.cat([torch.ones(1), 0.5 + torch.rand(T, generator=torch.Generator().manual_seed(9))])
    return make_module(H, 2, 8, T, _params(H), sigmas_norm=sn)


@functools.lru_cache(maxsize=None)
def _set(na, seed=23):
    fs = R.build_set(list(na), seed=seed)
    return SimpleNamespace(**{k: fs[k] for k in R.SET_KEYS})


def _times(B, k=0):
    t = np.random.default_rng(100 + k).integers(1, T + 1, size=B).astype(np.int32)
    t[0], t[-1] = 1, T
    return t


def _step(m, na, pool, call_id, accum=1, forward_only=False, k=0):
    """One train_step with device noise; returns (stats, out_parts, grad) -- grad None for the forward-only form."""
    from matinvent_amd import pretrain
    B = len(na)
    grad = None if forward_only else torch.zeros_like(m.decoder.theta)
    stats, parts = torch.zeros(4, device="cuda"), torch.full((B, 3), float("nan"), device="cuda")
    pretrain.train_step(m, _set(tuple(na)), _times(B, k), grad=grad, stats=stats, accum_steps=accum, seed=SEED, call_id=call_id, forward_only=forward_only,
                        out_parts=parts, pool=pool)
    return stats, parts, grad


def _same(a, b, what):
    for x, y, name in zip(a, b, ("stats", "out_parts", "grad")):
        if x is None and y is None:
            continue
        assert bool(torch.isfinite(y).all()), f"{what}: the classic {name} is not finite"
        assert torch.equal(x, y), f"{what}: {name} differs, max |d| = {float((x - y).abs().max())}, nan in pooled: {bool(torch.isnan(x).any())}"


def _table(lib, h, which):
    n = int(lib.mi_batch_index_table(h, which, None, 0))
    assert n >= 0, (which, n)
    out = np.full(max(n, 1), -7, dtype=np.int32)
    got = int(lib.mi_batch_index_table(h, which, out.ctypes.data_as(C.POINTER(C.c_int)), n))
    assert got == n, (which, got, n)
    return out[:n]


# ---- (1) tables -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("na", [[1], MIX, [171], [1 + g % 5 for g in range(300)]], ids=["one-atom", "mixed", "171-atoms", "300-crystals"])
def test_index_tables_of_a_pooled_handle_equal_the_classic_handles(na):
    m, lib = _module(), _lib.load()
    pool = _pool(poison=True)
    classic, pooled = m.make_batch(na), m.make_batch(na, pool=pool)
    try:
        N, E, Np = sum(na), sum(n * n for n in na), sum(n * (n - 1) // 2 for n in na)
        for cb in (classic, pooled):
            assert lib.mi_batch_num_nodes(cb._h) == N and lib.mi_batch_num_edges(cb._h) == E and cb.num_edges == E
        lens = dict(zip(TABLES, (len(na), N, N + 1, N, E, E, E, Np, Np, Np, Np, Np, len(na) + 1, len(na) + 1)))
        for which, name in enumerate(TABLES):
            a, b = _table(lib, classic._h, which), _table(lib, pooled._h, which)
            assert len(a) == lens[name] == len(b), (name, len(a), len(b), lens[name])
            assert np.array_equal(a, b), (name, np.flatnonzero(a != b)[:8])
        assert np.array_equal(_table(lib, pooled._h, 0), np.asarray(na)) and int(_table(lib, pooled._h, 2)[-1]) == E
        if na == [171]:
            assert Np == 14535
        assert lib.mi_batch_index_table(pooled._h, 14, None, 0) == _lib.MI_EINVAL
        small = np.zeros(1, dtype=np.int32)
        if N + 1 > 1:
            assert lib.mi_batch_index_table(pooled._h, 2, small.ctypes.data_as(C.POINTER(C.c_int)), 1) == _lib.MI_EINVAL
        # the lazily built index tensors of the pooled handle are the classic handle's
        assert torch.equal(pooled.num_atoms, classic.num_atoms) and torch.equal(pooled.batch, classic.batch)
    finally:
        classic.release()
        pooled.release()
    assert pool.stats()["live_handles"] == 0 and pool.stats()["bytes_in_use"] == 0
    pool.close()


# ---- (2) recycled, poisoned memory --------------------------------------------------------------------------------------------------

def test_recycled_poisoned_memory_gives_the_same_bits():
    """A step on [20] * 6 leaves its blocks in the pool; the step on [1, 7, 20, 3, 13] that follows takes them over (larger blocks for
    smaller requests, other buffers than before) and must give the classic handle's bits: statistics, per-crystal sums, the whole
    gradient -- with accum_steps = 1 and 3."""
    m = _module()
    pool = _pool(poison=True)
    _step(m, [20] * 6, pool, call_id=3)
    s0 = pool.stats()
    assert s0["bytes_in_use"] == 0 and s0["live_handles"] == 0 and s0["mallocs"] > 40 and s0["bytes_reserved"] > 0
    for accum in (1, 3):
        _same(_step(m, MIX, pool, call_id=7, accum=accum), _step(m, MIX, None, call_id=7, accum=accum), f"accum_steps = {accum}")
    s1 = pool.stats()
    assert s1["reuses"] > s0["reuses"] and s1["bytes_in_use"] == 0
    pool.close()


def _window_run(m, na, pool):
    """Three training forwards + backwards on one handle with a weight-gradient window of 2 (one automatic contraction, one flush):
    mi_batch_set_wgrad_window / mi_cspnet_forward_train / mi_cspnet_backward / mi_cspnet_wgrad_flush.  (mi_pretrain_micro_step refuses
    an open window for its taped form, so the window is exercised through the entries that own it.)"""
    from matinvent_amd.cspnet import _ptr, _stream
    lib, net = _lib.load(), m.decoder
    B, N = len(na), sum(na)
    g = torch.Generator().manual_seed(77)
    net.sync()
    cb = m.make_batch(na, pool=pool)
    grad = torch.zeros_like(net.theta)
    outs = []
    try:
        cb.set_wgrad_window(net, 2)
        for k in range(3):
            temb, types = torch.randn(B, net.latent_dim, generator=g).cuda(), torch.randn(N, 100, generator=g).cuda()
            frac, lat = torch.rand(N, 3, generator=g).cuda(), (torch.eye(3) * 5 + torch.randn(B, 3, 3, generator=g)).cuda().contiguous()
            pl, px, pt = torch.empty(B, 3, 3, device="cuda"), torch.empty(N, 3, device="cuda"), torch.empty(N, 100, device="cuda")
            _lib.check(lib.mi_cspnet_forward_train(net._h, cb._h, _ptr(temb), _ptr(types), _ptr(frac), _ptr(lat), _ptr(pl), _ptr(px), _ptr(pt), _stream()))
            dl, dx, dt = torch.randn(B, 3, 3, generator=g).cuda(), torch.randn(N, 3, generator=g).cuda(), torch.randn(N, 100, generator=g).cuda()
            _lib.check(lib.mi_cspnet_backward(net._h, cb._h, _ptr(dl), _ptr(dx), _ptr(dt), _ptr(grad), _stream()))
            outs += [pl, px, pt]
        assert lib.mi_batch_wgrad_pending(cb._h) == 1
        cb.wgrad_flush(net, grad)
        cb.set_wgrad_window(net, 0)
    finally:
        cb.release()
    return outs, grad


def test_a_weight_gradient_window_on_a_pooled_handle_gives_the_same_bits():
    m = _module()
    pool = _pool(poison=True)
    _step(m, [20] * 6, pool, call_id=3)
    po, pg = _window_run(m, MIX, pool)
    co, cg = _window_run(m, MIX, None)
    assert bool(torch.isfinite(cg).all()) and float(cg.abs().max()) > 0
    for k, (a, b) in enumerate(zip(po, co)):
        assert torch.equal(a, b), f"prediction {k}"
    assert torch.equal(pg, cg), f"max |d| = {float((pg - cg).abs().max())}, nan: {bool(torch.isnan(pg).any())}"
    assert pool.stats()["bytes_in_use"] == 0
    pool.close()


# ---- (3) the tape's plane-set branch ------------------------------------------------------------------------------------------------

def test_the_plane_set_branch_of_the_tape_on_recycled_poisoned_memory():
    """256-wide network, 22 crystals x 20 atoms: E = 8 800 >= 8192 and Np = 4 180 >= 4096, so the tape allocates and clears M1pl_l, DmPl
    and DpPl -- on the pool's stream for the pooled handle -- after a step on 24 x 20 left its blocks in the poisoned pool."""
    assert 22 * 400 >= 8192 > 20 * 400 and 22 * 190 >= 4096 > 21 * 190
    m = _module(256)
    pool = _pool(poison=True)
    _step(m, [20] * 24, pool, call_id=3)
    _same(_step(m, [20] * 22, pool, call_id=9), _step(m, [20] * 22, None, call_id=9), "22 x 20 at H = 256")
    assert pool.stats()["bytes_in_use"] == 0
    pool.close()


# ---- (4) inference and forward-only ---------------------------------------------------------------------------------------------------

def _forward_twice(m, na, pool):
    B, N = len(na), sum(na)
    g = torch.Generator().manual_seed(31)
    temb, types = torch.randn(B, m.decoder.latent_dim, generator=g).cuda(), torch.randn(N, 100, generator=g).cuda()
    frac, lat = torch.rand(N, 3, generator=g).cuda(), (torch.eye(3) * 5 + torch.randn(B, 3, 3, generator=g)).cuda()
    cb = m.make_batch(na, pool=pool)
    try:
        with torch.no_grad():
            first = m.decoder(temb, types, frac, lat, None, batch=cb)
            second = m.decoder(temb, types, (frac + 0.25) % 1.0, lat, None, batch=cb)
    finally:
        cb.release()
    return list(first) + list(second)


@pytest.mark.parametrize("H", [64, 256])
def test_inference_forward_and_forward_only_step_on_a_pooled_handle(H):
    """mi_cspnet_forward twice on one handle (H = 256: the fused node chain, whose first inference forward allocates PQ0 from the pool),
    and train_step(forward_only=True): bit-equal to the classic handle."""
    m = _module(H)
    pool = _pool(poison=True)
    _step(m, [20] * 6, pool, call_id=3, forward_only=True)
    for k, (a, b) in enumerate(zip(_forward_twice(m, MIX, pool), _forward_twice(m, MIX, None))):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b), f"H = {H}: output {k}"
    _same(_step(m, MIX, pool, call_id=0, forward_only=True), _step(m, MIX, None, call_id=0, forward_only=True), f"H = {H} forward-only")
    assert pool.stats()["bytes_in_use"] == 0
    pool.close()


# ---- (5) no allocation after warm-up ------------------------------------------------------------------------------------------------

def test_no_allocation_after_the_warm_up_step():
    """One step on 8 crystals with the maximal counts, then 20 distinct mini-batches whose counts are elementwise <= the first (the
    construction of tests/test_gpu_pretrain.py's memory test).  Every request of a later handle is <= the corresponding request of the
    warm-up handle and the set of requests is the same or a subset; any larger block may serve any smaller request, so smallest-feasible
    placement finds the assignment that exists: the hipMalloc count does not move."""
    from matinvent_amd import pretrain
    from matinvent_amd.data import CrystalData
    m = _module()
    gen = torch.Generator().manual_seed(0)

    def batch(k):
        na = [20, 19, 18, 17, 16, 16, 5, 3] if k == 0 else [20, 19, 18, 17, 1 + k % 16, 1 + k // 16, 5, 3]
        return [CrystalData(torch.rand(n, 3, generator=gen), torch.randint(1, 95, (n,), generator=gen), 4 + 6 * torch.rand(1, 3, generator=gen),
                            70 + 40 * torch.rand(1, 3, generator=gen)) for n in na], na
    pool = _pool(poison=True)
    seen = set()

    def run(k):
        items, na = batch(k)
        assert tuple(na) not in seen and all(a <= b for a, b in zip(na, batch(0)[1]))
        seen.add(tuple(na))
        pretrain.train_step(m, pretrain._as_batch(items, m.device), pretrain.draw_times(len(na), T, 0, k, SEED), seed=SEED, pool=pool)
        s = pool.stats()
        assert s["bytes_in_use"] == 0 and s["live_handles"] == 0, (k, s)
        return s
    s1 = run(0)
    torch.cuda.synchronize()
    free_1 = torch.cuda.mem_get_info()[0]
    torch.cuda.synchronize()
    slack = abs(free_1 - torch.cuda.mem_get_info()[0])
    for k in range(1, 21):
        s = run(k)
        assert s["mallocs"] == s1["mallocs"] and s["frees"] == 0 and s["bytes_reserved"] == s1["bytes_reserved"], (k, s, s1)
    torch.cuda.synchronize()
    free_21 = torch.cuda.mem_get_info()[0]
    assert abs(free_21 - free_1) <= slack, (free_1, free_21, slack)
    assert s["reuses"] >= 20 * 40 and s["bytes_high_water"] <= s1["bytes_high_water"]
    assert bool(torch.isfinite(m.decoder.theta.grad).all())
    m.decoder.theta.grad = None
    pool.close()


# ---- (6) the cap ----------------------------------------------------------------------------------------------------------------------

def test_a_cap_below_one_handles_need_fails_cleanly_and_leaves_the_pool_usable():
    m = _module()
    probe = _pool()
    cb = m.make_batch([20] * 6, pool=probe)
    need = probe.stats()["bytes_in_use"]
    cb.release()
    probe.close()
    assert need > 1 << 20
    pool = _pool(max_bytes=need // 2)
    with pytest.raises(_lib.MIError) as ei:
        m.make_batch([20] * 6, pool=pool)
    assert ei.value.code == _lib.MI_ENOMEM and "cap" in str(ei.value)
    s = pool.stats()
    assert s["bytes_in_use"] == 0 and s["live_handles"] == 0 and s["max_bytes"] == need // 2 and s["bytes_reserved"] <= need // 2
    pool.trim()                                         # later pool calls still work: what the failed create left cached is freed ...
    assert pool.stats()["bytes_reserved"] == 0 and pool.stats()["frees"] == s["mallocs"] > 0
    small = m.make_batch([2, 1, 3], pool=pool)          # ... and a handle that fits is created
    assert pool.stats()["live_handles"] == 1 and 0 < pool.stats()["bytes_in_use"] <= need // 2
    small.release()
    pool.close()


def test_a_cap_between_one_and_two_handles_trims_the_cached_blocks_for_another_shape():
    """[20] * 6, released, then [24] * 6 (every request at least as large; the edge-sized ones outgrow every cached block).  An uncapped
    probe pool runs the sequence first: it ends with R bytes reserved, of which the second handle holds less -- both handles make the same
    list of requests, so every fresh block of the second leaves a cached block of the first unused.  Under a cap of R - 512 the same
    sequence meets the cap at a fresh block, the cached blocks are freed (the hipFree count rises) and the create succeeds: what it then
    allocates afresh is never larger than the cached block it took in the probe."""
    m = _module()
    A, Bp = [20] * 6, [24] * 6
    alone = _pool()
    cb = m.make_batch(Bp, pool=alone)
    need_b = alone.stats()["bytes_in_use"]
    cb.release()
    alone.close()
    probe = _pool()
    m.make_batch(A, pool=probe).release()
    need_a = probe.stats()["bytes_reserved"]
    cb = m.make_batch(Bp, pool=probe)
    sp = probe.stats()
    cb.release()
    probe.close()
    cap = sp["bytes_reserved"] - 512
    assert sp["frees"] == 0 and sp["bytes_reserved"] - sp["bytes_in_use"] >= 512     # a cached block of the first handle stayed unused
    assert need_a < need_b <= cap < 2 * need_b, (need_a, need_b, cap)               # the cap lies between one handle's need and twice that
    pool = _pool(max_bytes=cap)
    m.make_batch(A, pool=pool).release()
    s0 = pool.stats()
    assert s0["frees"] == 0 and s0["bytes_reserved"] == need_a
    cb = m.make_batch(Bp, pool=pool)                                                 # succeeds
    s1 = pool.stats()
    assert s1["frees"] > 0 and s1["live_handles"] == 1 and s1["bytes_reserved"] <= cap, s1
    lib = _lib.load()
    assert np.array_equal(_table(lib, cb._h, 0), np.asarray(Bp))                     # ... and the handle is whole
    cb.release()
    pool.close()


# ---- (7) fit ----------------------------------------------------------------------------------------------------------------------------

def test_fit_with_a_handle_pool_gives_the_weights_of_fit_without():
    from matinvent_amd import pretrain
    from matinvent_amd.data import CrystalData
    na = [4, 2, 6, 3, 1, 7, 5, 2, 8, 3, 4, 6]

    def data(seed):
        fs = R.build_set(na, seed=seed)
        off = np.concatenate([[0], np.cumsum(na)])
        return [CrystalData(fs["frac_coords"][off[i]:off[i + 1]], fs["atom_types"][off[i]:off[i + 1]], fs["lengths"][i:i + 1], fs["angles"][i:i + 1])
                for i in range(len(na))]
    train, val = data(11), data(12)[:5]
    sn = torch.cat([torch.ones(1), 0.5 + torch.rand(T, generator=torch.Generator().manual_seed(9))])
    runs = []
    for hp in (False, True):
        m = make_module(64, 2, 8, T, _params(64), sigmas_norm=sn)
        cfg = dict(lr=1e-3, epochs=3, batch_size=3, accum_steps=2, max_grad_norm=1.0, handle_pool=hp)
        stats = pretrain.fit(m, train, cfg, val_list=val, seed=SEED, log=lambda *_: None)
        runs.append((m.decoder.theta.detach().clone(), stats, m.__dict__.get("handle_pool_stats")))
    assert len(runs[0][1]) == 3 and np.isfinite([v for d in runs[0][1] for v in d.values()]).all()
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert runs[0][2] is None
    ps = runs[1][2]
    assert ps["live_handles"] == 0 and ps["bytes_in_use"] == 0 and ps["reuses"] > ps["mallocs"] > 0


# ---- (8) refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals():
    m, lib = _module(), _lib.load()
    pool = _pool()
    cb = m.make_batch(MIX, pool=pool)
    before = pool.stats()
    try:
        # the sampler and a trajectory entry: MI_EINVAL from their first line, before an argument is read or anything is enqueued
        rc = lib.mi_sampler_run(m.decoder._h, cb._h, None, 10, 10, 0, None, 0, None, None, None, None, None, None)
        assert rc == _lib.MI_EINVAL and b"pooled" in lib.mi_last_error()
        rc = lib.mi_traj_logprob(m.decoder._h, cb._h, cb._h, None, None, 10, *([None] * 12), 0, None)
        assert rc == _lib.MI_EINVAL and b"pooled" in lib.mi_last_error()
        assert lib.mi_batch_set_time_map(cb._h, None, 0) == _lib.MI_EINVAL and b"pooled" in lib.mi_last_error()
        # a supported entry on another stream than the pool's: refused on its first line, by comparing the two handles -- the stream is
        # not touched, so a value that is no stream at all will do (creating one here would shift the hardware queues that the streams of
        # every later test in the process are mapped to)
        out = torch.zeros(len(MIX), 4, device="cuda")
        rc = lib.mi_structure_check(cb._h, C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(pool.stream + 64))
        assert rc == _lib.MI_EINVAL and b"stream" in lib.mi_last_error()
        assert pool.stats() == before
        # the pool with a live handle
        assert lib.mi_pool_destroy(pool._handle()) == _lib.MI_ESTATE and b"alive" in lib.mi_last_error()
        with pytest.raises(_lib.MIError) as ei:
            pool.close()
        assert ei.value.code == _lib.MI_ESTATE and pool.stats()["live_handles"] == 1
        # the knn style
        with pytest.raises(_lib.MIError) as ei:
            from matinvent_amd.cspnet import CrystalBatch
            CrystalBatch(m.decoder, MIX, edge_style="knn", pool=pool)
        assert ei.value.code == _lib.MI_EINVAL and pool.stats()["live_handles"] == 1
    finally:
        cb.release()
    pool.close()
    with pytest.raises(RuntimeError, match="closed"):
        pool.stats()
