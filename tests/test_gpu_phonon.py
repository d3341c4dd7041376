"""The phonon kernels on the device against the numpy restatement tests/phonon_ref64.py, bit for bit (include/matinvent_hip_phonon.h;
DESIGN 51).  No network is involved: the rows Gc fed in are those of synthetic crystals defined by their force constants
(Gc = float32(g0 +- h Phi row), widened), written where mi_vib_collect would write them.  Every output of mi_phonon_fc, mi_phonon_dynmat
and mi_phonon_thermo and the eigenvalues of mi_sym_eigvals are compared on NaN-poisoned workspaces -- Phi, the masks, asym, every matrix,
herm, eigenvalues, sweeps, the pair means, frequencies, counts, the zero-point energy, the lowest frequency and its q, pair_gap -- to
equality.  c_v alone carries a tolerance: it goes through expm1, whose device version may differ from the host's in the last place
(CV_RTOL of tests/test_vib_host.py, derived there); the weights 1 and 2 multiply exactly and the division by their sum is IEEE."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import phonon_ref64 as R
from tests.test_phonon_host import (DET_MIN, GRID_Q, GRID_WEIGHTS, H, KERNEL_CASES, NU_CUT, Q_LIST, Q_WEIGHTS, TEMPS, TIE_TOL, compare, grid_models, kernel_models,
                                    model_rows, reference)
from tests.test_vib_host import EIGVALSH_BOUND

pytestmark = pytest.mark.gpu

POISON = -7.0


def _p(cap=1 << 30):
    return SimpleNamespace(predictor=SimpleNamespace(device="cuda"), delta=H, per_atom=True, temperatures=TEMPS, nu_cut=NU_CUT, det_min=DET_MIN, tie_tol=TIE_TOL,
                           batch_size=256, workspace_cap=cap, p=0, scale=lambda: 1.0)


def _run(models, rows, reps, q, weights, no_lds=0, cap=1 << 30):
    """mi_phonon_fc, then per range of items mi_phonon_dynmat and mi_sym_eigvals, then mi_phonon_thermo, on a list of synthetic crystals of
    one reps whose rows Gc are written into a NaN-poisoned workspace.  Returns (device results per crystal, the number of ranges)."""
    from matinvent_amd import phonons as PH
    p = _p(cap)
    na = [md["Ns"] for md in models]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    src = PH.source_arrays(p, (t(np.concatenate([md["frac"] for md in models])), t(np.stack([md["lat"] for md in models])), torch.zeros(sum(na), 100).cuda()), na,
                           np.concatenate([md["mass_all"] for md in models]), reps, PH.phase_table(q, reps), weights, no_lds)
    o = src["ws_off_host"]
    ws = np.full(int(o[-1]), np.nan)
    for b, (md, Gc) in enumerate(zip(models, rows)):
        ws[o[b]:o[b] + Gc.size] = Gc.reshape(-1)
    src["ws"].copy_(t(ws))
    for k in ("mats", "evals", "lam", "freqs", "herm_item", "asym", "c_v", "zpe", "min_freq", "herm", "pair_gap"):
        src[k].fill_(float("nan"))
    if src["work"] is not None:
        src["work"].fill_(float("nan"))
    for k in ("sweeps", "eig_status", "fc_status", "n_imag", "n_zero", "min_q", "sweeps_max", "status"):
        src[k].fill_(-9)
    PH.enqueue_fc(p, src)
    sizes, mat_off, E = src["sizes"].cpu().numpy(), src["mat_off"].cpu().numpy(), [None] * src["T"]
    for start, stop in src["cuts"]:
        PH.enqueue_dynmat(p, src, start, stop)
        PH.enqueue_eigvals(p, src, start, stop, no_lds)
        mats = src["mats"].cpu().numpy()
        for it in range(start, stop):
            E[it] = mats[mat_off[it]:mat_off[it] + sizes[it] ** 2].reshape(sizes[it], sizes[it]).copy()
    PH.enqueue_thermo(p, src)
    ws, eo, Q = src["ws"].cpu().numpy(), src["ev_off_host"], src["Q"]
    host = {k: src[k].cpu().numpy() for k in ("asym", "fc_status", "sweeps", "eig_status", "herm_item", "evals", "lam", "freqs", "c_v", "zpe", "n_imag", "n_zero",
                                              "min_freq", "min_q", "herm", "pair_gap", "sweeps_max", "status")}
    out = []
    for b, md in enumerate(models):
        n, Ns = src["prim"][b], md["Ns"]
        items = range(b * Q, (b + 1) * Q)
        masks = ws[o[b] + 27 * n * Ns:o[b] + 27 * n * Ns + (n * Ns + 1) // 2].view(np.int32)[:n * Ns].reshape(n, Ns)
        out.append(dict(Phi=ws[o[b] + 18 * n * Ns:o[b] + 27 * n * Ns].reshape(3 * n, 3 * Ns), masks=masks, E=[E[it] for it in items],
                        evals=[host["evals"][eo[it]:eo[it + 1]] for it in items], sweeps=[host["sweeps"][it] for it in items],
                        eig_status=[host["eig_status"][it] for it in items], herm_item=host["herm_item"][b * Q:(b + 1) * Q],
                        lam=host["lam"][eo[b * Q] // 2:eo[(b + 1) * Q] // 2].reshape(Q, 3 * n), freqs=host["freqs"][eo[b * Q] // 2:eo[(b + 1) * Q] // 2].reshape(Q, 3 * n),
                        **{k: host[k][b] for k in ("asym", "fc_status", "c_v", "zpe", "n_imag", "n_zero", "min_freq", "min_q", "herm", "pair_gap", "sweeps_max", "status")}))
    return out, len(src["cuts"])


def _lapack(dev, n, what):
    """The device's eigenvalues are LAPACK's of the device's matrix within the Jacobi bound."""
    for E, ev in zip(dev["E"], dev["evals"]):
        assert np.abs(ev - np.linalg.eigvalsh(E)).max() <= EIGVALSH_BOUND * 6 * n * 2.0 ** -53 * np.linalg.norm(E, 2), what


@pytest.mark.parametrize("case,no_lds", [(k, 0) for k in range(len(KERNEL_CASES))] + [(4, 1)])
def test_kernels_bit_for_bit_over_the_cases(case, no_lds):
    """(n, reps) = (1, (1, 1, 1)): every D(q) exactly zero; (1, (2, 1, 1)), (2, (2, 2, 2)), (3, (3, 1, 2)): every pair coupled, tied
    wrap-around images; (20, (2, 1, 1)): order 120, the largest family in LDS, also with the LDS path forced off -- the same bits;
    (22, (1, 1, 1)): order 132, in global memory.  At Gamma, a zone-boundary point, a point with irrational components and the (2, 1, 1)
    mesh."""
    n, reps = KERNEL_CASES[case]
    md = kernel_models()[case]
    assert (md["n"], md["reps"]) == (n, reps) and (6 * n <= 128) == (case != 5)
    dev, _ = _run([md], [model_rows("kernel", case)], reps, Q_LIST, Q_WEIGHTS, no_lds=no_lds)
    ref = reference("kernel", case)
    compare(ref, dev[0], n, f"case {case} no_lds={no_lds}")
    assert int(dev[0]["status"]) == R.OK and int(dev[0]["n_imag"]) == 0
    _lapack(dev[0], n, case)
    if case == 0:
        assert all(not E.any() for E in dev[0]["E"]) and not dev[0]["c_v"].any() and int(dev[0]["n_zero"]) == 3 * int(Q_WEIGHTS.sum())
    if case in (1, 2):
        assert max(bin(int(v)).count("1") for v in dev[0]["masks"].reshape(-1)) >= 2   # tied images


def _grid_batch():
    """300 crystals of 1 to 3 atoms at (2, 1, 1), the same three-atom crystal at positions 0, 150 and 299."""
    kinds = list(range(300))
    for pos in (0, 150, 299):
        kinds[pos] = 2
    models = [grid_models()[k] for k in kinds]
    assert len(models) == 300 and {md["n"] for md in models} == {1, 2, 3} and models[0]["n"] == 3
    return kinds, models, [model_rows("grid", k) for k in kinds]


def test_three_hundred_small_crystals_and_batch_independence():
    """Every crystal of the batch against its own restatement, the item list cut into several ranges by a small workspace cap; and a
    crystal's outputs are the same alone and at positions 0, 150 and 299."""
    kinds, models, rows = _grid_batch()
    dev, ranges = _run(models, rows, (2, 1, 1), GRID_Q, GRID_WEIGHTS, cap=64 << 10)
    assert ranges > 4
    for b, k in enumerate(kinds):
        compare(reference("grid", k), dev[b], models[b]["n"], f"grid {b}")
        assert int(dev[b]["status"]) == R.OK
    alone, one = _run([models[0]], [rows[0]], (2, 1, 1), GRID_Q, GRID_WEIGHTS)
    assert one == 1
    same = lambda a, b: np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    for pos in (0, 150, 299):
        for k, v in alone[0].items():
            if isinstance(v, list):
                assert all(same(x, y) for x, y in zip(v, dev[pos][k])), (pos, k)
            else:
                assert same(v, dev[pos][k]), (pos, k)
            if k == "c_v":
                assert np.array_equal(v, dev[pos][k]), pos   # (the same device arithmetic: equal, not close)


def test_bad_input_fails_its_crystal_alone():
    """A NaN gradient element and a flat cell beside healthy neighbours: each is BAD_INPUT with NaN downstream and counts -1, and the
    neighbours keep the bits they have alone (their own restatement)."""
    g = grid_models()
    spoiled = model_rows("grid", 5).copy()
    spoiled[3, 4] = np.nan
    flat = dict(g[8], lat=np.zeros((3, 3), np.float32))
    models, rows, kinds = [g[2], g[5], g[1], flat, g[0]], [model_rows("grid", 2), spoiled, model_rows("grid", 1), model_rows("grid", 8), model_rows("grid", 0)], [2, None, 1, None, 0]
    dev, _ = _run(models, rows, (2, 1, 1), GRID_Q, GRID_WEIGHTS)
    for b, k in enumerate(kinds):
        if k is not None:
            compare(reference("grid", k), dev[b], models[b]["n"], f"healthy {b}")
            assert int(dev[b]["status"]) == R.OK
            continue
        ref = R.analyze(models[b], rows[b], GRID_Q, GRID_WEIGHTS, TEMPS, NU_CUT, H, TIE_TOL, DET_MIN)
        compare(ref, dev[b], models[b]["n"], f"bad {b}")
        d = dev[b]
        assert int(d["status"]) == int(d["fc_status"]) == R.BAD_INPUT and np.isnan(d["Phi"]).all() and not d["masks"].any() and np.isnan(d["asym"])
        assert all(np.isnan(E).all() for E in d["E"]) and all(np.isnan(e).all() for e in d["evals"]) and [int(s) for s in d["eig_status"]] == [R.BAD_INPUT] * 2
        assert np.isnan(d["c_v"]).all() and np.isnan(d["zpe"]) and np.isnan(d["freqs"]).all() and np.isnan(d["min_freq"]) and np.isnan(d["herm"]) and np.isnan(d["pair_gap"])
        assert int(d["n_imag"]) == int(d["n_zero"]) == int(d["min_q"]) == int(d["sweeps_max"]) == -1


def test_bad_arguments_are_refused_by_name_and_nothing_is_written():
    from matinvent_amd import _lib, phonons as PH
    from matinvent_amd.cspnet import _stream
    lib, p = _lib.load(), _p()
    md, Gc = grid_models()[2], model_rows("grid", 2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    state = (t(md["frac"]), t(md["lat"][None]), torch.zeros(md["Ns"], 100).cuda())
    # reps that does not divide the atom count; a primitive cell whose order exceeds the solver's
    with pytest.raises(_lib.MIError, match="reps does not divide the atom count"):
        PH.source_arrays(p, state, [md["Ns"]], md["mass_all"], (2, 2, 1), PH.phase_table(GRID_Q, (2, 2, 1)), GRID_WEIGHTS)
    with pytest.raises(_lib.MIError, match="6 n > MI_EIG_MAX_M"):
        PH.ws_layout([129], (1, 1, 1))
    # a q-table of the wrong length
    src = PH.source_arrays(p, state, [md["Ns"]], md["mass_all"], (2, 1, 1), PH.phase_table(GRID_Q, (2, 1, 1)), GRID_WEIGHTS)
    src["ws"].fill_(float("nan"))
    src["ws"][:Gc.size].copy_(t(Gc.reshape(-1).copy()))
    PH.enqueue_fc(p, src)
    for k in ("mats", "herm_item"):
        src[k].fill_(POISON)
    src["table_len"] -= 1
    with pytest.raises(_lib.MIError, match="the q-table has 47 doubles"):
        PH.enqueue_dynmat(p, src, 0, src["T"])
    torch.cuda.synchronize()
    assert bool((src["mats"] == POISON).all()) and bool((src["herm_item"] == POISON).all())
    src["table_len"] += 1
    # a device-side count that reps does not divide: BAD_INPUT for that crystal, nothing addressed
    a = _lib.PhononFcArgs(PH._at(src["ws"]), PH._at(src["ws_off"]), PH._at(src["node_off"]), PH._at(src["mass"]), PH._at(src["frac"]), PH._at(src["lat"]),
                          PH._at(src["asym"]), PH._at(src["fc_status"]), H, TIE_TOL, DET_MIN, (C.c_int * 3)(2, 2, 1), 1, md["Ns"])
    keep = src["ws"].clone()
    _lib.check(lib.mi_phonon_fc(C.byref(a), _stream()), "mi_phonon_fc")
    assert int(src["fc_status"][0]) == R.BAD_INPUT and bool(torch.isnan(src["asym"][0])) and torch.equal(src["ws"].view(torch.int64), keep.view(torch.int64))
    # ... and the healthy call still gives the restatement
    PH.enqueue_spectrum(p, src)
    ref = reference("grid", 2)
    assert int(src["status"][0]) == R.OK and np.array_equal(src["freqs"].cpu().numpy().reshape(2, 9), ref["freqs"])
