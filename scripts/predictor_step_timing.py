"""Cost of one property-predictor training micro-step on the benchmark network (H 512, L 6, F 128): mi_scalar_micro_step beside
mi_pretrain_micro_step on the same kept batch handle in the same process, alternating, and the predictor's inference throughput.

    python scripts/predictor_step_timing.py [--iters 20] [--json OUT]

Two sets: 256 crystals x 20 atoms, and the reference's default-size fine-tune set (18 crystals, SampleDataset atom counts).  Prints one
JSON line per set: ms per micro-step of both entries (two alternating rounds each), their ratio, the predictor's forward-only form, and --
at 256 x 20 -- `predict` crystals per second (host wall clock over whole calls, handles created per mini-batch as predict does).  The
predictor's flat vector starts with the module's trunk weights, so both entries run the same network.  The script asserts nothing about
the outcome."""
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


def measure(agent, model, na, iters, g, with_predict):
    from matinvent_amd import _lib, predictor, pretrain
    from matinvent_amd.cspnet import _ptr, _stream
    from matinvent_amd.data import CrystalBatchData, CrystalData
    T = agent.beta_scheduler.timesteps
    data = [CrystalData(torch.rand(n, 3, generator=g), torch.randint(1, 95, (n,), generator=g), 4 + 6 * torch.rand(1, 3, generator=g),
                        70 + 40 * torch.rand(1, 3, generator=g), properties={"y": float(torch.randn((), generator=g))}) for n in na]
    B, N, P = len(na), sum(na), model.P
    batch = CrystalBatchData(data).to("cuda")
    lib = _lib.load()
    f = lambda x: x.to("cuda", torch.float32).contiguous()
    lengths, angles, frac0, at = f(batch.lengths), f(batch.angles), f(batch.frac_coords), batch.atom_types.to("cuda", torch.int32).contiguous()
    table, freqs = pretrain.schedule_table(agent), agent.time_embedding.freqs
    grad_a, st4 = torch.zeros_like(agent.decoder.theta), torch.zeros(4, device="cuda")
    grad_p, stp = torch.zeros_like(model.flat), torch.zeros(predictor.stats_len(P), device="cuda")
    yhat, have = model.normalizer(data)
    cb = agent.make_batch(na)   # ONE kept handle for both entries (same H and L: the two nets' handles are interchangeable)
    step = [0]

    def pre(forward_only=False):
        step[0] += 1
        th = pretrain.draw_times(B, T, 0, step[0], 0)
        t_dev = torch.from_numpy(th).to("cuda")
        agent.decoder.sync()
        _lib.check(lib.mi_pretrain_micro_step(agent.decoder._h, cb._h, _ptr(lengths), _ptr(angles), _ptr(frac0), _ptr(at), _ptr(freqs),
                                              th.ctypes.data_as(C.POINTER(C.c_int)), _ptr(t_dev), _ptr(table), T, 0, step[0], None, None, None,
                                              agent.cost_lattice, agent.cost_coord, agent.cost_type, B, N, 1, None if forward_only else _ptr(grad_a),
                                              _ptr(st4), None, _stream()), "mi_pretrain_micro_step")

    def sca(forward_only=False):
        predictor.train_step(model, batch, yhat=yhat, have=have, grad=grad_p, stats=stp, handle=cb, forward_only=forward_only)

    ms_pre = [timed(pre, iters)]
    ms_sca = [timed(sca, iters)]
    ms_pre.append(timed(pre, iters))
    ms_sca.append(timed(sca, iters))
    ms_fwd = timed(lambda: sca(True), iters)
    cb.release()
    row = dict(crystals=B, atoms=N, edges=sum(n * n for n in na), iters=iters, ms_pretrain_micro_step=[round(v, 3) for v in ms_pre],
               ms_scalar_micro_step=[round(v, 3) for v in ms_sca], scalar_over_pretrain=round(sum(ms_sca) / sum(ms_pre), 4),
               ms_scalar_forward_only=round(ms_fwd, 3), finite=bool(torch.isfinite(grad_p).all() and torch.isfinite(stp).all()))
    if with_predict:
        model.predict(data, batch_size=256)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(max(1, iters // 4)):
            model.predict(data, batch_size=256)
        torch.cuda.synchronize()
        row["predict_crystals_per_s"] = round(max(1, iters // 4) * B / (time.perf_counter() - t0), 1)
    return row


def main():
    from matinvent_amd.predictor import PropertyPredictor
    from matinvent_amd.sampling import SampleDataset
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    H, L, F, T = 512, 6, 128, 1000
    hp = O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F)
    P = O.init_params(hp, seed=3, head_scale=0.1)
    g = torch.Generator().manual_seed(5)
    agent = make_module(H, L, F, T, P)
    model = PropertyPredictor(["y"], hidden_dim=H, num_layers=L, time_dim=256, num_freqs=F, ln=True, device="cuda", seed=3)
    model.load_state_dict(dict(agent.decoder.state_dict(), **{k: v for k, v in model.state_dict().items() if k.startswith("scalar_out.")}))
    np.random.seed(0)
    rows = []
    for name, na in (("256x20", [20] * 256), ("reference-default-18", [int(n) for n in SampleDataset(18).num_atoms])):
        row = dict(set=name, **measure(agent, model, na, a.iters, g, with_predict=name == "256x20"))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
