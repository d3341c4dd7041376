"""Cost of one supervised training micro-step on the benchmark network (H 512, L 6, F 128, T = 1000): mi_pretrain_micro_step beside
mi_ft_micro_step on the same set in the same process, alternating, and the cost of creating plus releasing a mini-batch's batch handle
(what pretrain.train_step pays per micro-step for not keeping handles) as a share of the step.

    python scripts/pretrain_step_timing.py [--iters 20] [--pool] [--json OUT]

Two sets: 256 crystals x 20 atoms, and the reference's default-size fine-tune set (18 crystals, SampleDataset atom counts).  Prints one
JSON line per set: ms per micro-step of both entries on kept handles (device noise; the fine-tune entry with its frozen prior's forward
forked onto a second stream, as ft_step runs it), the forward-only form, ms per handle create + release (host wall clock, the device idle),
ms per pretrain.train_step (which does both, and allocates the tape inside the fresh handle), and the ratios:
handle_share = create + release / train_step, overhead_share = (train_step - the entry on a kept handle) / train_step.  The script asserts nothing about the outcome.
--pool adds, per set: ms per pretrain.train_step on a POOLED handle in steady state (pool.HandlePool, warmed up; host wall
clock like the unpooled one, measured alternating with it -- unpooled, pooled, unpooled, pooled -- in this process), ms per pooled handle
create + release alone, their ratios to the unpooled figures, and the pool's statistics."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import diffcsp_oracle as O  # noqa: E402
from tests.gpu_util import make_module  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def wall(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def measure(agent, prior, na, iters, g, with_pool=False):
    from matinvent_amd import _lib, finetune, pretrain, streams
    from matinvent_amd.cspnet import _ptr, _stream
    from matinvent_amd.data import CrystalBatchData, CrystalData
    T = agent.beta_scheduler.timesteps
    data = [CrystalData(torch.rand(n, 3, generator=g), torch.randint(1, 95, (n,), generator=g), 4 + 6 * torch.rand(1, 3, generator=g),
                        70 + 40 * torch.rand(1, 3, generator=g)) for n in na]
    B, N = len(na), sum(na)
    batch = CrystalBatchData(data)
    batch.reward = torch.rand(B, generator=g)
    batch = batch.to("cuda")
    agent.shard_offsets = prior.shard_offsets = (0, 0)
    aux = streams.concurrent_streams(2, "cuda")[1]
    grad, st3, st4 = torch.zeros_like(agent.decoder.theta), torch.zeros(3, device="cuda"), torch.zeros(4, device="cuda")
    lib = _lib.load()
    cb = agent.make_batch(na)   # a kept handle: the entry alone
    f = lambda x: x.to("cuda", torch.float32).contiguous()
    lengths, angles, frac0, at = f(batch.lengths), f(batch.angles), f(batch.frac_coords), batch.atom_types.to("cuda", torch.int32).contiguous()
    table, freqs = pretrain.schedule_table(agent), agent.time_embedding.freqs
    step = [0]

    def entry(forward_only):
        step[0] += 1
        th = pretrain.draw_times(B, T, 0, step[0], 0)
        t_dev = torch.from_numpy(th).to("cuda")
        agent.decoder.sync()
        _lib.check(lib.mi_pretrain_micro_step(agent.decoder._h, cb._h, _ptr(lengths), _ptr(angles), _ptr(frac0), _ptr(at), _ptr(freqs),
                                              th.ctypes.data_as(C.POINTER(C.c_int)), _ptr(t_dev), _ptr(table), T, 0, step[0], None, None, None,
                                              agent.cost_lattice, agent.cost_coord, agent.cost_type, B, N, 1, None if forward_only else _ptr(grad),
                                              _ptr(st4), None, _stream()), "mi_pretrain_micro_step")

    def ft():
        step[0] += 1
        finetune._fused_micro_step(agent, prior, batch, step[0] % T, None, 0.025, B, 10, grad, st3, aux_stream=aux)

    def handle():
        agent.make_batch(na).release()

    def whole():
        step[0] += 1
        pretrain.train_step(agent, batch, pretrain.draw_times(B, T, 0, step[0], 0), grad=grad, stats=st4)

    ms_ft = timed(ft, iters)
    ms_pre = timed(lambda: entry(False), iters)
    ms_ft2 = timed(ft, iters)
    ms_pre2 = timed(lambda: entry(False), iters)
    ms_fwd = timed(lambda: entry(True), iters)
    ms_handle = wall(handle, iters)
    ms_whole = wall(whole, iters)
    pre, ftm = 0.5 * (ms_pre + ms_pre2), 0.5 * (ms_ft + ms_ft2)
    cb.release()
    extra = {}
    if with_pool:
        from matinvent_amd.pool import HandlePool
        pool = HandlePool()

        def whole_pooled():
            step[0] += 1
            pretrain.train_step(agent, batch, pretrain.draw_times(B, T, 0, step[0], 0), grad=grad, stats=st4, pool=pool)

        def handle_pooled():
            agent.make_batch(na, pool=pool).release()

        cl, po = [], []
        for _ in range(2):
            cl.append(wall(whole, iters))
            po.append(wall(whole_pooled, iters))
        ms_hp = wall(handle_pooled, iters)
        ps = pool.stats()
        pool.close()
        extra = dict(ms_train_step_wall_alternating=[round(v, 3) for v in cl], ms_train_step_pooled_wall=[round(v, 3) for v in po],
                     pooled_over_unpooled_train_step=round(sum(po) / sum(cl), 4), ms_pooled_handle_create_release=round(ms_hp, 3),
                     pooled_over_kept_handle_entry=round(0.5 * sum(po) / pre, 4), pool_stats=ps)
    return dict(crystals=B, atoms=N, edges=sum(n * n for n in na), iters=iters, ms_ft_micro_step=[round(ms_ft, 3), round(ms_ft2, 3)],
                ms_pretrain_micro_step=[round(ms_pre, 3), round(ms_pre2, 3)], pretrain_over_ft=round(pre / ftm, 4),
                ms_pretrain_forward_only=round(ms_fwd, 3), ms_handle_create_release=round(ms_handle, 3), ms_train_step_wall=round(ms_whole, 3),
                handle_share_of_train_step=round(ms_handle / ms_whole, 4),
                overhead_share_of_train_step=round((ms_whole - pre) / ms_whole, 4), finite=bool(torch.isfinite(grad).all() and torch.isfinite(st4).all()),
                **extra)


def main():
    from matinvent_amd.sampling import SampleDataset
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pool", action="store_true", help="also time train_step on pooled handles (DESIGN 39)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    H, L, F, T = 512, 6, 128, 1000
    hp = O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F)
    P = O.init_params(hp, seed=3, head_scale=0.1)
    g = torch.Generator().manual_seed(5)
    agent = make_module(H, L, F, T, {k: v + 0.002 * torch.randn(v.shape, generator=g) for k, v in P.items()})
    prior = make_module(H, L, F, T, P)
    prior.requires_grad_(False)
    np.random.seed(0)
    rows = []
    for name, na in (("256x20", [20] * 256), ("reference-default-18", [int(n) for n in SampleDataset(18).num_atoms])):
        row = dict(set=name, **measure(agent, prior, na, a.iters, g, with_pool=a.pool))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
