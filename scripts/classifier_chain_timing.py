"""Cost of a classifier-guided reverse chain on the benchmark network (H 512, L 6, F 128, T = 1000 schedule, S = 250 respaced steps; a
predictor of the same shape, one property): ms per reverse step of a guided chain (every step guided, lattice and coordinates) against the
plain chain of the same batch on one stream, alternating in one process -- plain, guided, plain, ... -- so that the yardstick is the plain
chain of that process; and the cost of one guided step's additions, split into the seed's inference forward, the taped forward with the
data-only backward (mi_scalar_input_grad) and the shift.

    python scripts/classifier_chain_timing.py [--steps 20] [--rounds 3] [--json OUT]

64 and 256 crystals x 20 atoms.  A chain measurement is the host wall clock of `steps` reverse steps from the top of the view's grid
(sample(t_start=S, t_stop=S - steps)) with the device drained on both sides, after a warm-up call per form; per configuration the median
over `rounds` rounds.  The parts are timed with device events over 20 repetitions each on the state the chain starts from.  The
expectation to compare with: one plain step, plus the parts.  Prints one JSON line per configuration.  The script asserts nothing about
the outcome."""
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
    from matinvent_amd import classifier as CG, predictor as PR
    T, S = 1000, 250
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
    guide = CG.ClassifierGuidance(pred, "y", mode="max", scale=1.0, max_shift=0.05)
    rows = []
    for B in (64, 256):
        na = [20] * B
        box = Box(na)

        def run(c):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            view.sample(box, step_lr=5e-6, seed=1, t_start=S, t_stop=S - a.steps, streams=1, **({} if c is None else {"classifier": c}))
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / a.steps
        forms = {"plain": None, "guided": guide}
        for c in forms.values():
            run(c)
        ms = {k: [] for k in forms}
        for _ in range(a.rounds):
            for k, c in forms.items():
                ms[k].append(run(c))
        med = {k: statistics.median(x) for k, x in ms.items()}
        # one guided step's additions, in their parts
        f = view.sample(box, step_lr=5e-6, seed=1, t_start=S, t_stop=S)[0]
        state = (f["frac_coords"], f["lattices"], f["atom_types"])
        ph = guide.handle(na)
        tk = int(view.time_map[S])
        d_out = torch.ones(B, 1, device="cuda")
        out, gx, gl, _ = PR.input_gradient(pred, state, ph, tk, d_out=d_out, types=False)
        t_seed = _device_ms(lambda: PR.guide_seed(pred, PR.forward_state(pred, state, ph, tk), "y", "max"))
        t_grad = _device_ms(lambda: PR.input_gradient(pred, state, ph, tk, d_out=d_out, types=False))
        scratch = tuple(x.clone() for x in state)
        t_shift = _device_ms(lambda: CG.shift(guide, ph, scratch, (gx, gl, None), (0.0, 0.0, 0.0)))
        parts = t_seed + t_grad + t_shift
        row = dict(crystals=B, atoms=20, grid=S, steps=a.steps, rounds=a.rounds, ms_per_step={k: round(x, 3) for k, x in med.items()},
                   all_ms_per_step={k: [round(y, 3) for y in x] for k, x in ms.items()}, guided_over_plain=round(med["guided"] / med["plain"], 4),
                   step_parts_ms=dict(seed_forward=round(t_seed, 4), taped_forward_and_data_backward=round(t_grad, 4), shift=round(t_shift, 4)),
                   expected_over_plain=round(1.0 + parts / med["plain"], 4))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
