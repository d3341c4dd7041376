"""The vibration kernels on the device against the numpy restatement tests/vib_ref64.py, bit for bit (include/matinvent_hip_vib.h; DESIGN
47).  No network is involved: the gradients fed in are float64 analytic values of the synthetic spring energy at the device's own displaced
coordinates, cast to float32.  Every intermediate is compared -- displaced coordinates, Gc, the reduced matrices, asym, eigenvalues, sweeps,
frequencies, counts, the zero-point energy -- to equality.  c_v alone carries a tolerance: it goes through expm1, whose device version may
differ from the host's in the last place (CV_RTOL below); sqrt and division are IEEE on both sides."""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import vib_ref64 as R
from tests.test_vib_host import ATOM_COUNTS, CV_RTOL, EIGVALSH_BOUND, EIG_SIZES, H, NU_CUT, PER_ATOM, SCALE, TEMPS, eig_matrices, grid_crystals, kernel_crystals

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _plain_model():
    """A predictor whose handles the synthetic-gradient tests run on (the kernels read the handle's offsets alone)."""
    from matinvent_amd import predictor as PR
    return PR.PropertyPredictor(["energy"], hidden_dim=64, num_layers=2, time_dim=256, num_freqs=8, ln=True, device="cuda", seed=3)


def _v(batch_size=256):
    return SimpleNamespace(predictor=_plain_model(), delta=H, per_atom=PER_ATOM, temperatures=TEMPS, nu_cut=NU_CUT, det_min=1e-3, batch_size=batch_size, p=0,
                           scale=lambda: SCALE)


def _run(crystals, no_lds=0, spoil=None, batch_size=256):
    """The five entries on a list of synthetic crystals: displace per chunk, the analytic gradient at the device's coordinates, collect,
    dynmat, eigvals, thermo.  spoil = [(crystal, copy, atom, d)]: those gradient elements are NaN.  Returns (device results per crystal, the
    float32 gradients that were fed in)."""
    from matinvent_amd import _lib, vibrations as VB
    from matinvent_amd.cspnet import _stream
    lib = _lib.load()
    v = _v(batch_size)
    na = [sp["n"] for sp in crystals]
    z = np.concatenate([np.full(n, 1 + k % 90) for k, n in enumerate(na)])
    types = np.zeros((z.size, 100), np.float32)
    types[np.arange(z.size), z - 1] = 1.0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    src = VB.source_arrays(v, (t(np.concatenate([sp["frac"] for sp in crystals])), t(np.stack([sp["lat"] for sp in crystals])), t(types)), na,
                           np.concatenate([sp["mass"] for sp in crystals]))
    src["ws"].fill_(float("nan"))   # (whatever is not written shows)
    g_fed = [np.empty((6 * n, n, 3), np.float32) for n in na]
    for ps, pc in VB.chunk_plan(na, batch_size):
        cna = [na[b] for b in ps]
        cb = v.predictor.make_batch(cna)
        bufs = VB.chunk_buffers(v, len(cna), sum(cna))
        for k in ("types", "frac", "lat"):
            bufs[k].fill_(-7.0)
        dps, dpc = t(ps.copy()), t(pc.copy())
        args = VB.chunk_args(v, src, dps, dpc, bufs)
        _lib.check(lib.mi_vib_displace(cb._h, C.byref(args), _stream()), "mi_vib_displace")
        x, l, ty = bufs["frac"].cpu().numpy(), bufs["lat"].cpu().numpy(), bufs["types"].cpu().numpy()
        off = np.concatenate([[0], np.cumsum(cna)])
        g = np.empty((off[-1], 3), np.float32)
        for k, (b, c) in enumerate(zip(ps, pc)):
            sp, rows = crystals[b], slice(off[k], off[k + 1])
            assert np.array_equal(x[rows], R.displace(sp["frac"], sp["lat"], int(c), H)), ("displaced coordinates", b, c)
            assert np.array_equal(l[k].reshape(3, 3), sp["lat"]) and np.array_equal(ty[rows], types[sum(na[:b]):sum(na[:b]) + na[b]]), ("copied rows", b, c)
            g[rows] = R.spring_gradient(sp, x[rows], sp["lat"])[1].astype(np.float32)
            for sb, sc, sa, sd in spoil or ():
                if (b, c) == (sb, sc):
                    g[off[k] + sa, sd] = np.nan
            g_fed[b][c] = g[rows]
        bufs["g_frac"].copy_(t(g))
        _lib.check(lib.mi_vib_collect(cb._h, C.byref(args), _stream()), "mi_vib_collect")
        torch.cuda.synchronize()
        cb.release()
    VB.enqueue_dynmat(v, src)
    VB.enqueue_eigvals(v, src, no_lds)
    VB.enqueue_thermo(v, src)
    ws, o, eo = src["ws"].cpu().numpy(), src["ws_off"].cpu().numpy(), src["ev_off_host"]
    host = {k: src[k].cpu().numpy() for k in ("asym", "dyn_status", "sweeps", "eig_status", "c_v", "zpe", "n_imag", "n_zero", "status", "evals", "freqs")}
    out = []
    for b, n in enumerate(na):
        M = 3 * n - 3
        out.append(dict(Gc=ws[o[b]:o[b] + 18 * n * n].reshape(6 * n, 3 * n), R=ws[o[b] + 27 * n * n:o[b] + 27 * n * n + M * M].reshape(M, M),
                        evals=host["evals"][eo[b]:eo[b + 1]], freqs=host["freqs"][eo[b]:eo[b + 1]],
                        **{k: host[k][b] for k in ("asym", "dyn_status", "sweeps", "eig_status", "c_v", "zpe", "n_imag", "n_zero", "status")}))
    return out, g_fed


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


_REF = {}


def _reference(sp, g):
    """The restatement of a crystal from the gradients that were fed in: computed once per (crystal, gradients), shared, left unchanged."""
    hit = _REF.get(id(sp))
    if hit is None or not np.array_equal(hit[0], g, equal_nan=True):
        hit = _REF[id(sp)] = (g.copy(), R.analyze(sp, H, SCALE, PER_ATOM, TEMPS, NU_CUT, g_copies=g))
    return hit[1]


def _compare(crystals, dev, g_fed, what):
    """Every crystal, every output."""
    worst = 0.0
    for b, (sp, d, g) in enumerate(zip(crystals, dev, g_fed)):
        ref = _reference(sp, g)
        for k in ("Gc", "R", "asym", "evals", "freqs", "zpe"):
            assert _same(d[k], ref[k]), (what, b, sp["n"], k, d[k], ref[k])
        assert int(d["sweeps"]) == ref["sweeps"] and int(d["status"]) == ref["status"] and int(d["dyn_status"]) == (R.OK if ref["status"] == R.NO_CONVERGENCE else ref["status"]), (what, b, d["sweeps"], ref["sweeps"], d["status"], ref["status"])
        assert int(d["n_imag"]) == ref["n_imag"] and int(d["n_zero"]) == ref["n_zero"], (what, b)
        if ref["status"] == R.OK:
            err = np.abs(d["c_v"] - ref["c_v"])
            rel = float((err / np.where(ref["c_v"] > 0, ref["c_v"], 1.0)).max())
            worst = max(worst, rel)
            assert (err <= CV_RTOL * ref["c_v"]).all(), (what, b, d["c_v"], ref["c_v"])
            if sp["n"] == 1:
                assert not d["c_v"].any() and d["zpe"] == 0.0 and d["evals"].size == 0
            else:
                lap = np.linalg.eigvalsh(d["R"])
                assert np.abs(d["evals"] - lap).max() <= EIGVALSH_BOUND * (3 * sp["n"] - 3) * 2.0 ** -53 * np.linalg.norm(d["R"], 2), (what, b)
        else:
            assert np.isnan(d["c_v"]).all() and np.isnan(d["zpe"]) and np.isnan(d["freqs"]).all() and int(d["n_imag"]) == int(d["n_zero"]) == -1
    if os.environ.get("MI_TOL_REPORT"):
        print(f"TOL vib {what}: c_v device vs restatement, largest relative difference {worst:.3e} (allowed {CV_RTOL:.3e}: expm1); everything else equal")


@pytest.mark.parametrize("no_lds", [0, 1])
def test_kernels_bit_for_bit_over_the_atom_counts(no_lds):
    """Atom counts 1 (no modes), 2, 3 (odd and even order), 20, 43 (order 126: the largest in LDS), 44 (order 129: the smallest in global
    memory), and a crystal of isotropic springs whose every level is three-fold; with the LDS path and forced off it: the same bits."""
    crystals = kernel_crystals()
    assert [sp["n"] for sp in crystals][:len(ATOM_COUNTS)] == list(ATOM_COUNTS) == [1, 2, 3, 20, 43, 44]
    dev, g = _run(crystals, no_lds=no_lds)
    _compare(crystals, dev, g, f"counts no_lds={no_lds}")
    deg = dev[-1]["evals"]
    assert np.all(dev[-1]["status"] == R.OK) and deg.size == 12 and np.abs(deg.reshape(4, 3) - deg.reshape(4, 3).mean(axis=1, keepdims=True)).max() < 1e-4 * deg.max()


def test_three_hundred_small_crystals():
    crystals = grid_crystals()
    assert len(crystals) == 300 and {sp["n"] for sp in crystals} == {1, 2, 3}
    dev, g = _run(crystals, batch_size=1000)
    _compare(crystals, dev, g, "grid")


def test_bad_input_fails_its_crystal_alone():
    """A NaN gradient element in a three-atom crystal; and two crystals of ONE atom, which have no matrix element to carry a bad input to
    the solver -- one with a NaN gradient, one in a flat cell: each is BAD_INPUT with NaN outputs and counts -1, and the others keep the
    bits they have alone."""
    flat = dict(kernel_crystals()[0], lat=np.zeros((3, 3), np.float32))
    crystals = kernel_crystals()[1:4] + [kernel_crystals()[0], flat, grid_crystals()[0]]   # 2, 3, 20, 1, 1 (flat), 1 atoms
    assert [sp["n"] for sp in crystals] == [2, 3, 20, 1, 1, 1]
    dev, g = _run(crystals, spoil=[(1, 7, 2, 1), (3, 4, 0, 2)])
    for b in (1, 3, 4):
        assert int(dev[b]["status"]) == R.BAD_INPUT == int(dev[b]["dyn_status"]) and np.isnan(dev[b]["R"]).all() and np.isnan(dev[b]["asym"]), b
        assert np.isnan(dev[b]["c_v"]).all() and np.isnan(dev[b]["zpe"]) and int(dev[b]["n_imag"]) == int(dev[b]["n_zero"]) == -1, b
    assert [int(dev[b]["status"]) for b in (0, 2, 5)] == [R.OK] * 3 and not dev[5]["c_v"].any()
    _compare(crystals, dev, g, "bad input")   # (the others against their own references: the bits of a crystal alone)


@pytest.mark.parametrize("no_lds", [0, 1])
def test_sym_eigvals_alone(no_lds):
    """mi_sym_eigvals on its own: random symmetric matrices of order 1, 2, 3, 57, 126, 129, a diagonal one (0 sweeps), kron(I_3, S) (an
    exactly three-fold spectrum), an empty one and one with an infinite element, in one ragged batch."""
    from matinvent_amd import _lib
    from matinvent_amd.vibrations import _at
    from matinvent_amd.cspnet import _stream
    mats = eig_matrices()
    sizes = np.array([m.shape[0] for m in mats], np.int32)
    assert [int(s) for s in sizes[:len(EIG_SIZES)]] == list(EIG_SIZES) == [1, 2, 3, 57, 126, 129]
    off = np.concatenate([[0], np.cumsum(sizes.astype(np.int64) ** 2)])
    eo = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    flat = t(np.concatenate([m.reshape(-1) for m in mats]))
    keep = flat.clone()
    work, ev = torch.full_like(flat, float("nan")), torch.full((int(eo[-1]),), -7.0, dtype=torch.float64, device="cuda")
    d_off, d_sz, d_eo = t(off[:-1]), t(sizes), t(eo[:-1])
    sw, st = torch.full((len(mats),), -9, dtype=torch.int32, device="cuda"), torch.full((len(mats),), -9, dtype=torch.int32, device="cuda")
    a = _lib.SymEigArgs(_at(flat), _at(d_off), _at(d_sz), _at(work), None, _at(ev), _at(d_eo), _at(sw), _at(st), len(mats), int(sizes.max()), no_lds)
    _lib.check(_lib.load().mi_sym_eigvals(C.byref(a), _stream()), "mi_sym_eigvals")
    assert torch.equal(flat, keep)   # the input is read only
    ev, sw, st = ev.cpu().numpy(), sw.cpu().numpy(), st.cpu().numpy()
    for b, m in enumerate(mats):
        want, sweeps, status = R.jacobi(m)
        got = ev[eo[b]:eo[b + 1]]
        assert _same(got, want) and int(sw[b]) == sweeps and int(st[b]) == status, (b, m.shape, sw[b], sweeps, st[b], status)
        if status == R.OK and m.shape[0]:
            assert np.abs(got - np.linalg.eigvalsh(m)).max() <= EIGVALSH_BOUND * m.shape[0] * 2.0 ** -53 * np.linalg.norm(m, 2), b
    k = len(EIG_SIZES)
    assert sw[k] == 0 and st[k] == R.OK and _same(ev[eo[k]:eo[k + 1]], np.sort(np.diag(mats[k])))   # the diagonal one
    tri = ev[eo[k + 1]:eo[k + 2]].reshape(-1, 3)
    assert st[k + 1] == R.OK and np.abs(tri - tri[:, :1]).max() <= 2 * EIGVALSH_BOUND * mats[k + 1].shape[0] * 2.0 ** -53 * np.linalg.norm(mats[k + 1], 2)
    assert st[k + 3] == R.BAD_INPUT and np.isnan(ev[eo[k + 3]:eo[k + 4]]).all()
    # a work array is demanded exactly where one is needed
    a.work = None
    rc = _lib.load().mi_sym_eigvals(C.byref(a), _stream())
    assert rc == _lib.MI_EINVAL and b"work array" in _lib.load().mi_last_error()


def test_a_bad_plan_entry_writes_nothing():
    """A plan entry outside the source, a copy index outside 0 .. 6 n - 1 and an atom count that is not the source crystal's: neither
    displace nor collect writes for them, and nothing is read through the bad index; the good entry beside them is written."""
    from matinvent_amd import _lib, vibrations as VB
    from matinvent_amd.cspnet import _stream
    lib, v = _lib.load(), _v()
    crystals = kernel_crystals()[1:3]   # 2 and 3 atoms
    na = [2, 3]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    src = VB.source_arrays(v, (t(np.concatenate([sp["frac"] for sp in crystals])), t(np.stack([sp["lat"] for sp in crystals])), torch.zeros(5, 100).cuda()), na,
                           np.concatenate([sp["mass"] for sp in crystals]))
    src["ws"].fill_(float("nan"))
    cna = [2, 3, 2, 3, 2]
    plan_src, plan_copy = np.array([0, 1, -1, 2, 1], np.int32), np.array([3, 18, 0, 0, 0], np.int32)   # good | copy 6 n | src < 0 | src = Bs | 2 atoms for 3
    cb = v.predictor.make_batch(cna)
    bufs = VB.chunk_buffers(v, len(cna), sum(cna))
    for k in ("types", "frac", "lat"):
        bufs[k].fill_(-7.0)
    bufs["g_frac"].zero_()
    dps, dpc = t(plan_src), t(plan_copy)
    args = VB.chunk_args(v, src, dps, dpc, bufs)
    _lib.check(lib.mi_vib_displace(cb._h, C.byref(args), _stream()), "mi_vib_displace")
    _lib.check(lib.mi_vib_collect(cb._h, C.byref(args), _stream()), "mi_vib_collect")
    x, l, ty, ws = bufs["frac"].cpu().numpy(), bufs["lat"].cpu().numpy(), bufs["types"].cpu().numpy(), src["ws"].cpu().numpy()
    cb.release()
    assert np.array_equal(x[:2], R.displace(crystals[0]["frac"], crystals[0]["lat"], 3, H)) and np.array_equal(l[0], crystals[0]["lat"]) and not ty[:2].any()
    assert (x[2:] == -7.0).all() and (l[1:] == -7.0).all() and (ty[2:] == -7.0).all()
    o = src["ws_off"].cpu().numpy()
    written = np.isfinite(ws)
    assert written[o[0] + 3 * 6:o[0] + 4 * 6].all() and not ws[o[0] + 3 * 6:o[0] + 4 * 6].any() and written.sum() == 6
