"""Cost of the Gamma-point vibration analysis on the benchmark network (a predictor of H 512, L 6, F 128, one property): the
whole analysis (vibrations.analyze_state: every chunk's displace + input gradient + collect, then dynmat, eigenvalues, thermodynamics)
beside the number of chunks x mi_scalar_input_grad on one chunk; the new kernels beside a torch restatement of the same steps (float64,
torch.linalg.eigvalsh in the eigen-solver's place); and mi_sym_eigvals alone at orders 57, 126, 129 and 510 beside torch.linalg.eigvalsh.

    python scripts/vib_timing.py [--rounds 3] [--json OUT]

64 and 256 crystals x 20 atoms, chunks of 256 copies, random weights (the cost does not depend on them).  The whole analysis is the host
wall clock with the device drained on both sides, after a warm-up call; per configuration the median over `rounds` rounds.  Single
launches are timed with device events.  Prints one JSON line per configuration.  The script asserts nothing about the outcome."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
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


def torch_analysis(Gc, mass, h, temps, nu_cut):
    """Steps 3 to 5 in torch ops for B crystals of one atom count n: Gc [B][6 n][3 n], mass [B][n], float64.  The translations are
    projected out with P = I - T T^T (three zero eigenvalues stay in the spectrum) and torch.linalg.eigvalsh takes the solver's place."""
    B, n = mass.shape
    H = (Gc[:, 0::2] - Gc[:, 1::2]) / (2 * h)
    H = 0.5 * (H + H.transpose(1, 2))
    blk = H.view(B, n, 3, n, 3)
    eye = torch.eye(n, device=H.device, dtype=torch.bool)[None, :, None, :, None]
    diag = -(blk.masked_fill(eye, 0.0)).sum(3)
    diag = 0.5 * (diag + diag.transpose(2, 3))
    idx = torch.arange(n, device=H.device)
    blk[:, idx, :, idx, :] = diag.permute(1, 0, 2, 3)
    m3 = mass.repeat_interleave(3, dim=1)
    D = H / (m3[:, :, None] * m3[:, None, :]).sqrt()
    T = torch.zeros(B, 3 * n, 3, device=H.device, dtype=H.dtype)
    for d in range(3):
        T[:, d::3, d] = mass.sqrt()
    T = T / T.norm(dim=1, keepdim=True)
    P = torch.eye(3 * n, device=H.device, dtype=H.dtype)[None] - T @ T.transpose(1, 2)
    lam = torch.linalg.eigvalsh(P @ D @ P)
    nu = torch.sign(lam) * lam.abs().sqrt() * 15.633304
    live = nu > nu_cut
    x = (nu[:, :, None] * 47.992430733662204 / temps[None, None, :]).clamp(min=1e-30)
    term = (x / torch.expm1(x)) * (x / -torch.expm1(-x))
    return torch.where(live[:, :, None], term, torch.zeros_like(term)).sum(1), 0.5 * torch.where(live, nu * 4.135667696923859e-3, torch.zeros_like(nu)).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from matinvent_amd import _lib, predictor as PR, vibrations as VB
    from matinvent_amd.cspnet import _ptr, _stream
    from matinvent_amd.vibrations import _at
    lib = _lib.load()
    pred = PR.PropertyPredictor(["energy"], hidden_dim=512, num_layers=6, time_dim=256, num_freqs=128, ln=True, device="cuda", seed=1)
    v = VB.Vibrations(pred, "energy", batch_size=256)
    rows = []
    for B in (64, 256):
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
        from matinvent_amd.structure import MASSES
        mass = np.asarray(MASSES)[z.numpy() + 1]
        keep = {}

        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            src = VB.analyze_state(v, (frac, lat, types), na, mass)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if "src" in keep:
                VB.release_handles(keep["src"])
            keep["src"] = src
            return ms
        run()
        whole_ms = statistics.median(run() for _ in range(a.rounds))
        src = keep["src"]
        chunks = len(VB.chunk_plan(na, v.batch_size))
        # one chunk: 256 copies of 20 atoms
        cna = [n] * 256
        cb = pred.make_batch(cna)
        bufs = VB.chunk_buffers(v, 256, 256 * n)
        ps, pc = VB.chunk_plan(na, v.batch_size)[0]
        dps, dpc = torch.from_numpy(ps.copy()).cuda(), torch.from_numpy(pc.copy()).cuda()
        args = VB.chunk_args(v, src, dps, dpc, bufs)
        pred.trunk.sync()
        _, W, bias = pred.head_slices()
        disp_ms = _device_ms(lambda: _lib.check(lib.mi_vib_displace(cb._h, C.byref(args), _stream())))
        grad_ms = _device_ms(lambda: _lib.check(lib.mi_scalar_input_grad(pred.trunk._h, cb._h, _ptr(bufs["types"]), _ptr(bufs["frac"]), _ptr(bufs["lat"]),
                                                                          _ptr(pred.time_freqs), None, 0, _ptr(W), _ptr(bias), 1, _ptr(bufs["d_out"]), _ptr(bufs["out"]),
                                                                          None, _ptr(bufs["g_frac"]), _ptr(bufs["g_lat"]), _stream())))
        coll_ms = _device_ms(lambda: _lib.check(lib.mi_vib_collect(cb._h, C.byref(args), _stream())))
        # (collect rewrote the first chunk's rows from the same gradients' last evaluation: the workspace still holds a whole analysis)
        dyn_ms = _device_ms(lambda: VB.enqueue_dynmat(v, src))
        eig_ms = _device_ms(lambda: VB.enqueue_eigvals(v, src))
        eig_global_ms = _device_ms(lambda: VB.enqueue_eigvals(v, src, no_lds=1))
        thermo_ms = _device_ms(lambda: VB.enqueue_thermo(v, src))
        o = src["ws_off"].cpu().numpy()
        Gc = torch.stack([src["ws"][o[b]:o[b] + 18 * n * n].view(6 * n, 3 * n) for b in range(B)])
        m2 = src["mass"].view(B, n)
        temps = torch.tensor(v.temperatures, dtype=torch.float64, device="cuda")
        torch_ms = _device_ms(lambda: torch_analysis(Gc, m2, v.delta, temps, v.nu_cut), reps=5)
        cv_t, _ = torch_analysis(Gc, m2, v.delta, temps, v.nu_cut)
        okm = src["status"] == 0
        dev = float((cv_t[okm] - src["c_v"][okm]).abs().max()) if bool(okm.any()) else float("nan")
        row = dict(kind="analysis", crystals=B, atoms=n, chunks=chunks, analysis_ms=round(whole_ms, 2), input_grad_ms_per_chunk=round(grad_ms, 3),
                   chunks_x_input_grad_ms=round(chunks * grad_ms, 2), displace_ms=round(disp_ms, 4), collect_ms=round(coll_ms, 4), dynmat_ms=round(dyn_ms, 4),
                   eigvals_ms=round(eig_ms, 4), eigvals_global_ms=round(eig_global_ms, 4), thermo_ms=round(thermo_ms, 4), torch_steps_3_to_5_ms=round(torch_ms, 3),
                   status_ok=int(okm.sum()), max_sweeps=int(src["sweeps"].max()), c_v_vs_torch_max_abs=dev)
        print(json.dumps(row), flush=True)
        rows.append(row)
        cb.release()
        VB.release_handles(src)
    # the eigen-solver alone
    for M, nb in ((57, 64), (126, 64), (129, 64), (510, 4)):
        gen = torch.Generator().manual_seed(M)
        A = torch.randn(nb, M, M, generator=gen, dtype=torch.float64)
        A = (0.5 * (A + A.transpose(1, 2))).cuda().contiguous()
        off = (torch.arange(nb, dtype=torch.int64) * M * M).cuda()
        eo = (torch.arange(nb, dtype=torch.int64) * M).cuda()
        sz = torch.full((nb,), M, dtype=torch.int32).cuda()
        work, ev = torch.empty_like(A), torch.empty(nb, M, dtype=torch.float64, device="cuda")
        sw, st = torch.empty(nb, dtype=torch.int32, device="cuda"), torch.empty(nb, dtype=torch.int32, device="cuda")
        args = _lib.SymEigArgs(_at(A), _at(off), _at(sz), _at(work), None, _at(ev), _at(eo), _at(sw), _at(st), nb, M, 0)
        reps = 1 if M > 200 else 5
        ms = _device_ms(lambda: _lib.check(lib.mi_sym_eigvals(C.byref(args), _stream())), reps=reps)
        t_ms = _device_ms(lambda: torch.linalg.eigvalsh(A), reps=reps)
        ref = torch.linalg.eigvalsh(A)
        row = dict(kind="eigvals", order=M, matrices=nb, in_lds=M <= _lib.EIG_LDS_MAX_M, jacobi_ms=round(ms, 3), torch_eigvalsh_ms=round(t_ms, 3),
                   sweeps=int(sw.max()), status_ok=int((st == 0).sum()),
                   dev_units=float(((ev - ref).abs().amax(1) / (M * 2.0 ** -53 * torch.linalg.matrix_norm(A, 2))).max()))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
