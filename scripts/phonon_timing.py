"""Cost of the q-mesh phonon analysis beside the Gamma path of a supercell, on the same records and the benchmark network (a predictor of
H 512, L 6, F 128, one property): phonons.analyze_state (home-cell displacements: 6 n copies of the supercell per crystal,
N = abc matrices of order 6 n) against vibrations.analyze_state on the replicated state (6 n N copies, one matrix of order 3 n N - 3), and
the new kernels and mi_sym_eigvals alone.

    python scripts/phonon_timing.py [--crystals 8] [--atoms 8] [--reps 2 2 2] [--rounds 3] [--json OUT]

Random weights and random cells (the cost does not depend on them), chunks of 256 copies, mesh = reps.  Each analysis is the host wall clock
with the device drained on both sides, after a warm-up call; the median over `rounds` rounds.  Single launches are timed with device
events; the two things an analysis is made of are timed on their own as well -- the handle of one chunk shape (host work, made inside
every call; the mesh path's shorter last chunk needs a second one) and mi_vib_run_chunk on one chunk of 256 copies -- so that the fall
of the gradient evaluations by N can be read beside the wall clock.  Prints one JSON line.  The script asserts nothing about the outcome."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _device_ms(fn, reps=5):
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
    ap.add_argument("--crystals", type=int, default=8)
    ap.add_argument("--atoms", type=int, default=8)
    ap.add_argument("--reps", type=int, nargs=3, default=[2, 2, 2])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from matinvent_amd import phonons as PH, predictor as PR, vibrations as VB
    from matinvent_amd.data import SimpleStructure
    from matinvent_amd.structure import MASSES, lattice_matrix, make_supercell
    pred = PR.PropertyPredictor(["energy"], hidden_dim=512, num_layers=6, time_dim=256, num_freqs=128, ln=True, device="cuda", seed=1)
    reps, B, n = tuple(a.reps), a.crystals, a.atoms
    N = reps[0] * reps[1] * reps[2]
    rng = np.random.default_rng(B)
    prim = [SimpleStructure((4.0 + rng.random(3)).tolist(), (85.0 + 10.0 * rng.random(3)).tolist(), rng.integers(1, 90, n).tolist(), rng.random((n, 3))) for _ in range(B)]
    big = [make_supercell(r, reps) for r in prim]
    z = np.array(sum((r.species for r in big), []))
    types = np.zeros((z.size, 100), np.float32)
    types[np.arange(z.size), z - 1] = 1.0
    state = (torch.from_numpy(np.concatenate([r.frac_coords for r in big]).astype(np.float32)).cuda(),
             torch.from_numpy(np.stack([lattice_matrix(r.lengths, r.angles) for r in big]).astype(np.float32)).cuda(), torch.from_numpy(types).cuda())
    na, mass = [n * N] * B, np.asarray(MASSES, dtype=np.float64)[z]
    p = PH.Phonons(pred, "energy", supercell=reps, mesh=reps, batch_size=256)
    v = VB.Vibrations(pred, "energy", batch_size=256)
    keep = {}

    def run(kind):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        src = PH.analyze_state(p, state, na, mass, reps) if kind == "mesh" else VB.analyze_state(v, state, na, mass)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if kind in keep:
            VB.release_handles(keep[kind])
        keep[kind] = src
        return ms

    out = {}
    for kind in ("mesh", "gamma"):
        run(kind)
        out[kind] = statistics.median(run(kind) for _ in range(a.rounds))
    src, old = keep["mesh"], keep["gamma"]
    copies_new, copies_old = 6 * n * B, 6 * n * N * B
    # what an analysis is made of: a handle per distinct chunk shape (host work, made inside every call) and a gradient evaluation per chunk
    import ctypes as C
    from matinvent_amd import _lib
    from matinvent_amd.cspnet import _ptr, _stream
    k256 = min(256, copies_new)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cb = pred.make_batch([n * N] * k256)
    torch.cuda.synchronize()
    handle_ms = (time.perf_counter() - t0) * 1e3
    bufs = VB.chunk_buffers(p, k256, k256 * n * N)
    ps, pc = VB.chunk_plan(src["prim"], 256)[0]   # (a full chunk of 256 copies, whatever the balanced plan of the analysis is)
    dps, dpc = torch.from_numpy(ps[:k256].copy()).cuda(), torch.from_numpy(pc[:k256].copy()).cuda()
    args = VB.chunk_args(p, src, dps, dpc, bufs)
    pred.trunk.sync()
    _, W, bias = pred.head_slices()
    chunk_ms = _device_ms(lambda: _lib.check(_lib.load().mi_vib_run_chunk(pred.trunk._h, cb._h, C.byref(args), _ptr(pred.time_freqs), _ptr(W), _ptr(bias), pred.P,
                                                                          _ptr(bufs["d_out"]), _ptr(bufs["out"]), _ptr(bufs["g_lat"]), _stream())), reps=3)
    torch.cuda.synchronize()
    cb.release()
    fc_ms = _device_ms(lambda: PH.enqueue_fc(p, src))
    (start, stop), = src["cuts"]
    dyn_ms = _device_ms(lambda: PH.enqueue_dynmat(p, src, start, stop))

    def dyn_eig():
        PH.enqueue_dynmat(p, src, start, stop)   # (the solver's LDS path leaves the matrices as they are; the pair keeps the timing honest on either path)
        PH.enqueue_eigvals(p, src, start, stop)
    eig_ms = _device_ms(dyn_eig) - dyn_ms
    thermo_ms = _device_ms(lambda: PH.enqueue_thermo(p, src))

    def old_tail():
        VB.enqueue_dynmat(v, old)
        VB.enqueue_eigvals(v, old)
        VB.enqueue_thermo(v, old)
    old_tail_ms = _device_ms(old_tail, reps=2)
    lam_new = np.sort((src["lam"].cpu().numpy()))
    row = dict(kind="phonon_timing", crystals=B, atoms=n, reps=list(reps), images=N, supercell_atoms=n * N, q_points=int(src["Q"]), items=int(src["T"]),
               matrix_order_mesh=6 * n, matrix_order_gamma=3 * n * N - 3, copies_mesh=copies_new, copies_gamma=copies_old,
               chunks_mesh=-(-copies_new // 256), chunks_gamma=-(-copies_old // 256), gradient_evaluation_ratio=copies_old / copies_new,
               analysis_ms_mesh=round(out["mesh"], 2), analysis_ms_gamma=round(out["gamma"], 2), analysis_ratio=round(out["gamma"] / out["mesh"], 2),
               handle_ms_per_chunk_shape=round(handle_ms, 1), run_chunk_ms=round(chunk_ms, 2), run_chunk_copies=k256,
               gradient_ms_mesh=round(chunk_ms * copies_new / k256, 1), gradient_ms_gamma=round(chunk_ms * copies_old / k256, 1), fc_ms=round(fc_ms, 4), dynmat_ms=round(dyn_ms, 4), eigvals_ms=round(eig_ms, 4), thermo_ms=round(thermo_ms, 4),
               behind_gradients_ms_mesh=round(fc_ms + dyn_ms + eig_ms + thermo_ms, 4), behind_gradients_ms_gamma=round(old_tail_ms, 3),
               status_ok_mesh=int((src["status"] == 0).sum()), status_ok_gamma=int((old["status"] == 0).sum()), sweeps_max_mesh=int(src["sweeps_max"].max()),
               sweeps_max_gamma=int(old["sweeps"].max()), lam_min_mesh=float(lam_new[0]), lam_max_mesh=float(lam_new[-1]))
    print(json.dumps(row), flush=True)
    VB.release_handles(src)
    VB.release_handles(old)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
