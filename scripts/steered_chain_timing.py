"""Cost of a steered reverse chain on the benchmark network (H 512, L 6, F 128, T = 1000 schedule, S = 250 respaced steps; a predictor of
the same shape, one property): ms per reverse step of a steered chain (K = 8 particles, an event every 10 steps) against the plain chain
of the same batch on one stream, alternating in one process -- plain, steered, plain, ... -- so that the yardstick is the plain chain of
that process; and the cost of one event, split into the predictor's forward on the state and the resampling (plan + gather).

    python scripts/steered_chain_timing.py [--steps 20] [--rounds 3] [--json OUT]

64 and 256 crystals x 20 atoms (8 and 32 groups of 8).  A chain measurement is the host wall clock of `steps` reverse steps from the top of
the view's grid (sample(t_start=S, t_stop=S - steps): steps / 10 events) with the device drained on both sides, after a warm-up call per
form; per configuration the median over `rounds` rounds.  The event's parts are timed with device events over 20 repetitions each on the
state the chain starts from.  Prints one JSON line per configuration.  The script asserts nothing about the outcome."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.gpu_util import Box, make_module  # noqa: E402


def _device_ms(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from matinvent_amd import predictor as PR, steering as ST
    T, S, K, every = 1000, 250, 8, 10
    torch.manual_seed(0)
    sn = torch.cat([torch.ones(1), torch.linspace(1.2, 0.4, T)])
    m = make_module(512, 6, 128, T, None, sigmas_norm=sn)
    with torch.no_grad():   # (small heads: the states stay finite over the steps measured)
        v = m.decoder.views()
        for k in ("coord_out.weight", "lattice_out.weight", "type_out.weight", "type_out.bias"):
            v[k].mul_(0.1)
    m.decoder.mark_dirty()
    pred = PR.PropertyPredictor(["y"], hidden_dim=512, num_layers=6, time_dim=256, num_freqs=128, ln=True, device="cuda", seed=1)
    pred.hparams["noised"] = PR.noised_spec(m)   # (random weights: the cost does not depend on them)
    view = m.respaced(S)
    steer = ST.Steering(pred, "y", mode="max", particles=K, scale=1.0, every=every)
    rows = []
    for B in (64, 256):
        na = steer.replicate([20] * (B // K))
        box = Box(na)

        def run(s):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            view.sample(box, step_lr=5e-6, seed=1, t_start=S, t_stop=S - a.steps, streams=1, **({} if s is None else {"steer": s}))
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / a.steps
        forms = {"plain": None, "steered": steer}
        for s in forms.values():
            run(s)
        ms = {k: [] for k in forms}
        for _ in range(a.rounds):
            for k, s in forms.items():
                ms[k].append(run(s))
        med = {k: statistics.median(x) for k, x in ms.items()}
        # one event, in its parts
        f = view.sample(box, step_lr=5e-6, seed=1, t_start=S, t_stop=S)[0]
        state = (f["frac_coords"], f["lattices"], f["atom_types"])
        other = tuple(torch.empty_like(x) for x in state)
        ph = steer.handle(na)
        out = torch.empty(B, 1, device="cuda")
        u_prev, logw = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
        anc, st = torch.empty(B, dtype=torch.int32, device="cuda"), torch.zeros(3, device="cuda")
        t_fwd = _device_ms(lambda: PR.forward_state(pred, state, ph, int(view.time_map[S - every]), out=out))
        t_res = _device_ms(lambda: ST.resample(steer, ph, out, S - every, 1, u_prev, logw, state, other, anc, st))
        event = t_fwd + t_res
        row = dict(crystals=B, atoms=20, particles=K, every=every, grid=S, steps=a.steps, rounds=a.rounds,
                   ms_per_step={k: round(x, 3) for k, x in med.items()}, all_ms_per_step={k: [round(y, 3) for y in x] for k, x in ms.items()},
                   steered_over_plain=round(med["steered"] / med["plain"], 4), event_ms=dict(predictor_forward=round(t_fwd, 4), resample_and_gather=round(t_res, 4)),
                   expected_over_plain=round(1.0 + event / med["plain"] / every, 4))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
