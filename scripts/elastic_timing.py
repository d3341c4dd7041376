"""Cost of the elastic-tensor analysis on the benchmark network (a predictor of H 512, L 6, F 128, one property): the whole
analysis (elasticity.analyze_state: every chunk's strain + ion relaxation + input gradient + collect, then the fit) beside the number of
gradient evaluations x mi_scalar_input_grad on one chunk, and the three new kernels alone.

    python scripts/elastic_timing.py [--rounds 3] [--json OUT]

64 and 256 crystals x 20 atoms, chunks of 256 copies, clamped ions and ion_steps = 3, random weights (the cost does not depend on them).
The whole analysis is the host wall clock with the device drained on both sides, after a warm-up call; per configuration the median over
`rounds` rounds.  Single launches are timed with device events.  Prints one JSON line per configuration.  The script asserts nothing about
the outcome."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _device_ms(fn, reps=10):
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from matinvent_amd import _lib, elasticity as EL, predictor as PR
    from matinvent_amd.cspnet import _ptr, _stream
    lib = _lib.load()
    pred = PR.PropertyPredictor(["energy"], hidden_dim=512, num_layers=6, time_dim=256, num_freqs=128, ln=True, device="cuda", seed=1)
    rows = []
    for B in (64, 256):
        for ion_steps in (0, 3):
            e = EL.Elasticity(pred, "energy", batch_size=256, ion_steps=ion_steps)
            n = 20
            na = [n] * B
            N = sum(na)
            g = torch.Generator().manual_seed(B)
            frac = torch.rand(N, 3, generator=g).cuda()
            lat = (5.0 * torch.eye(3)[None] + 0.3 * torch.randn(B, 3, 3, generator=g)).cuda()
            z = torch.randint(0, 100, (N,), generator=g)
            types = torch.zeros(N, 100)
            types[torch.arange(N), z] = 1.0
            types = types.cuda()
            keep = {}

            def run():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                src = EL.analyze_state(e, (frac, lat, types), na)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                if "src" in keep:
                    EL.release_handles(keep["src"])
                keep["src"] = src
                return ms
            run()
            whole_ms = statistics.median(run() for _ in range(a.rounds))
            src = keep["src"]
            plan = EL.chunk_plan(B, e.batch_size)
            chunks = len(plan)
            # one chunk: 256 copies of 20 atoms
            cna = [n] * 256
            cb = pred.make_batch(cna)
            bufs = EL.chunk_buffers(e, 256, 256 * n)
            ps, pc = plan[0]
            dps, dpc = torch.from_numpy(ps.copy()).cuda(), torch.from_numpy(pc.copy()).cuda()
            args = EL.chunk_args(e, src, dps, dpc, bufs, relaxed=False)
            pred.trunk.sync()
            _, W, bias = pred.head_slices()
            strain_ms = _device_ms(lambda: _lib.check(lib.mi_elastic_strain(cb._h, C.byref(args), _stream())))
            grad_ms = _device_ms(lambda: _lib.check(lib.mi_scalar_input_grad(pred.trunk._h, cb._h, _ptr(bufs["types"]), _ptr(bufs["frac"]), _ptr(bufs["lat"]),
                                                                              _ptr(pred.time_freqs), None, 0, _ptr(W), _ptr(bias), 1, _ptr(bufs["d_out"]), _ptr(bufs["out"]),
                                                                              None, _ptr(bufs["g_frac"]), _ptr(bufs["g_lat"]), _stream())))
            coll_ms = _device_ms(lambda: _lib.check(lib.mi_elastic_collect(cb._h, C.byref(args), _stream())))
            # (collect rewrote the first chunk's rows from the same gradients' last evaluation: the workspace still holds a whole analysis)
            fit_ms = _device_ms(lambda: EL.enqueue_fit(e, src))
            evals = chunks * (ion_steps + 1)
            new_ms = chunks * (strain_ms + coll_ms) + fit_ms
            status = src["status"].cpu()
            row = dict(kind="analysis", crystals=B, atoms=n, ion_steps=ion_steps, chunks=chunks, gradient_evaluations=evals, analysis_ms=round(whole_ms, 2),
                       input_grad_ms_per_chunk=round(grad_ms, 3), evaluations_x_input_grad_ms=round(evals * grad_ms, 2), strain_ms=round(strain_ms, 4),
                       collect_ms=round(coll_ms, 4), fit_ms=round(fit_ms, 4), new_kernels_ms=round(new_ms, 4), new_kernels_share=round(new_ms / whole_ms, 5),
                       status_ok=int((status == 0).sum()), status_singular=int((status == 2).sum()), n_unrelaxed_max=int(src["n_unrelaxed"].max()))
            print(json.dumps(row), flush=True)
            rows.append(row)
            cb.release()
            EL.release_handles(src)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
