"""The elasticity kernels on the device against the numpy restatement tests/elastic_ref64.py, bit for bit (include/matinvent_hip_elastic.h;
DESIGN 48).  No network is involved: the lattice gradients fed in are float64 analytic values of the synthetic spring energy at the
device's own strained lattices, cast to float32.  Every output of mi_elastic_strain, mi_elastic_collect and mi_elastic_fit is compared --
the copies' types, coordinates and lattices, the workspace rows, asym, C, S, stress0, pressure, asym_C, the moduli, the eigenvalues, cond
and the counts -- to equality, for every crystal.  No float64 operation of this unit turned out not to be bit-reproducible (there is no
transcendental function in it; sqrt and division are IEEE on both sides), so nothing carries a tolerance."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import elastic_ref64 as R
from tests.test_elastic_host import ATOM_COUNTS, DET_MIN, H, PER_ATOM, SCALE, grid_crystals, kernel_crystals

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _plain_model():
    """A predictor whose handles the synthetic-gradient tests run on (the kernels read the handle's offsets alone)."""
    from matinvent_amd import predictor as PR
    return PR.PropertyPredictor(["energy"], hidden_dim=64, num_layers=2, time_dim=256, num_freqs=8, ln=True, device="cuda", seed=3)


def _e(batch_size=256):
    return SimpleNamespace(predictor=_plain_model(), delta=H, per_atom=PER_ATOM, det_min=DET_MIN, batch_size=batch_size, p=0, ion_steps=0, scale=lambda: SCALE)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _types(na):
    z = np.concatenate([np.full(n, 1 + k % 90) for k, n in enumerate(na)])
    types = np.zeros((z.size, 100), np.float32)
    types[np.arange(z.size), z - 1] = 1.0
    return types


def _read(src):
    host = {k: src[k].cpu().numpy() for k in R.FIT_KEYS}
    ws = src["ws"].cpu().numpy()
    return [dict(rows=ws[b], C=host["C"][b].reshape(6, 6), S=host["S"][b].reshape(6, 6), moduli=host["moduli"][b].reshape(3, 5),
                 **{k: host[k][b] for k in R.FIT_KEYS if k not in ("C", "S", "moduli")}) for b in range(src["B"])]


def _run(crystals, spoil=None, batch_size=256, ists=None):
    """The three entries on a list of synthetic crystals: strain per chunk, the analytic lattice gradient at the device's lattices, collect,
    then fit.  spoil = [(crystal, copy, r, q)]: those gradient elements are NaN.  ists: per crystal, the 13 relaxation statuses handed to
    collect (None: clamped ions, no istate).  Returns (device results per crystal with the copies' lattices, the float32 gradients fed in)."""
    from matinvent_amd import _lib, elasticity as EL
    from matinvent_amd.cspnet import _stream
    lib, e = _lib.load(), _e(batch_size)
    na = [sp["n"] for sp in crystals]
    types = _types(na)
    noff = np.concatenate([[0], np.cumsum(na)])
    src = EL.source_arrays(e, (_t(np.concatenate([sp["frac"] for sp in crystals])), _t(np.stack([sp["lat"] for sp in crystals])), _t(types)), na)
    src["ws"].fill_(float("nan"))   # (whatever is not written shows)
    src["asym"].fill_(-3.0)
    g_fed = np.empty((len(na), R.COPIES, 3, 3), np.float32)
    lats = np.empty((len(na), R.COPIES, 3, 3), np.float32)
    for ps, pc in EL.chunk_plan(len(na), batch_size):
        cna = [na[b] for b in ps]
        cb = e.predictor.make_batch(cna)
        bufs = EL.chunk_buffers(e, len(cna), sum(cna))
        for k in ("types", "frac", "lat"):
            bufs[k].fill_(-7.0)
        if ists is not None:
            ist = np.zeros((len(cna), 3), np.int32)
            ist[:, 0] = [ists[b][c] for b, c in zip(ps, pc)]
            bufs["istate"].copy_(_t(ist))
        dps, dpc = _t(ps.copy()), _t(pc.copy())
        args = EL.chunk_args(e, src, dps, dpc, bufs, relaxed=ists is not None)
        _lib.check(lib.mi_elastic_strain(cb._h, C.byref(args), _stream()), "mi_elastic_strain")
        x, l, ty = bufs["frac"].cpu().numpy(), bufs["lat"].cpu().numpy(), bufs["types"].cpu().numpy()
        off = np.concatenate([[0], np.cumsum(cna)])
        g = np.empty((len(cna), 3, 3), np.float32)
        for k, (b, c) in enumerate(zip(ps, pc)):
            sp, rows = crystals[b], slice(off[k], off[k + 1])
            assert np.array_equal(l[k], R.strain(sp["lat"], int(c), H, DET_MIN), equal_nan=True), ("strained lattice", b, c)
            assert np.array_equal(x[rows], sp["frac"]) and np.array_equal(ty[rows], types[noff[b]:noff[b + 1]]), ("copied rows", b, c)
            with np.errstate(invalid="ignore", over="ignore"):
                g[k] = R.spring_lattice_gradient(sp, l[k])[1].astype(np.float32)
            for sb, sc, sr, sq in spoil or ():
                if (b, c) == (sb, sc):
                    g[k, sr, sq] = np.nan
            g_fed[b, c], lats[b, c] = g[k], l[k]
        bufs["g_lat"].copy_(_t(g))
        _lib.check(lib.mi_elastic_collect(cb._h, C.byref(args), _stream()), "mi_elastic_collect")
        torch.cuda.synchronize()
        cb.release()
    EL.enqueue_fit(e, src)
    out = _read(src)
    for b, o in enumerate(out):
        o["lats"] = lats[b]
    return out, g_fed, src


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _compare(crystals, dev, g_fed, what, ists=None):
    """Every crystal, every output."""
    for b, (sp, d) in enumerate(zip(crystals, dev)):
        ref = R.analyze(sp, H, SCALE, PER_ATOM, DET_MIN, g_copies=g_fed[b], lats=d["lats"], ist=None if ists is None else ists[b])
        for k in ("rows",) + R.FIT_KEYS:
            assert _same(d[k], ref[k]), (what, b, sp["n"], k, d[k], ref[k])
        if ref["status"] == R.BAD_INPUT:
            assert all(np.isnan(d[k]).all() for k in ("C", "S", "stress0", "pressure", "asym", "asym_C", "moduli", "evals", "cond")), (what, b)
            assert int(d["n_negative"]) == int(d["n_unrelaxed"]) == -1
        else:
            assert np.isfinite(d["C"]).all() and np.array_equal(d["C"], d["C"].T) and (np.diff(d["evals"]) >= 0).all(), (what, b)


def _sym_eigvals(src):
    """mi_sym_eigvals on the device's own C."""
    from matinvent_amd import _lib
    from matinvent_amd.cspnet import _stream
    from matinvent_amd.vibrations import _at
    B = src["B"]
    off = _t(np.arange(B, dtype=np.int64) * 36)
    sizes, eo = _t(np.full(B, 6, np.int32)), _t(np.arange(B, dtype=np.int64) * 6)
    ev = torch.full((B, 6), -7.0, dtype=torch.float64, device="cuda")
    sw, st = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    a = _lib.SymEigArgs(_at(src["C"]), _at(off), _at(sizes), None, None, _at(ev), _at(eo), _at(sw), _at(st), B, 6, 0)
    _lib.check(_lib.load().mi_sym_eigvals(C.byref(a), _stream()), "mi_sym_eigvals")
    return ev


def test_kernels_bit_for_bit_over_the_atom_counts():
    """Atom counts 1, 2, 171 (more rows than a workgroup's threads cover in one pass of the type copy: 171 x 25 float4 over 256 threads; an
    odd count), 20 and 3 in one batch; the eigenvalues are mi_sym_eigvals' on the same C."""
    crystals = kernel_crystals()
    assert [sp["n"] for sp in crystals] == list(ATOM_COUNTS) == [1, 2, 171, 20, 3]
    dev, g, src = _run(crystals)
    _compare(crystals, dev, g, "counts")
    assert [int(d["status"]) for d in dev] == [R.OK] * 5 and all(int(d["n_unrelaxed"]) == 0 for d in dev)
    assert torch.equal(src["evals"].view(torch.int64), _sym_eigvals(src).view(torch.int64))
    # a crystal's bits do not depend on its place or its batch: the same five, reversed, in chunks of 5 (13 is no multiple of 5)
    rev, g2, _ = _run(crystals[::-1], batch_size=5)
    _compare(crystals[::-1], rev, g2, "reversed")
    for d, r in zip(dev, rev[::-1]):
        for k in ("rows",) + R.FIT_KEYS:
            assert _same(d[k], r[k]), k


def test_three_hundred_small_crystals():
    crystals = grid_crystals()
    assert len(crystals) == 300 and {sp["n"] for sp in crystals} == {1, 2, 3}
    dev, g, src = _run(crystals, batch_size=1000)
    _compare(crystals, dev, g, "grid")
    assert all(int(d["status"]) == R.OK for d in dev)
    assert torch.equal(src["evals"].view(torch.int64), _sym_eigvals(src).view(torch.int64))


def test_bad_input_fails_its_crystal_alone():
    """A NaN g_lat element in one copy of a three-atom crystal and of a one-atom crystal, a flat cell of three atoms and of one: each is
    BAD_INPUT with NaN outputs and counts -1, and the others keep the bits they have alone.  A lattice-independent energy is SINGULAR with
    C = 0 and the Voigt values kept."""
    k = kernel_crystals()
    flat3, flat1 = dict(k[4], lat=np.zeros((3, 3), np.float32)), dict(k[0], lat=np.zeros((3, 3), np.float32))
    free = R.make_springs(2, 5, flat=True)
    crystals = [k[1], k[4], k[3], k[0], flat3, flat1, grid_crystals()[0], free, k[4]]
    assert [sp["n"] for sp in crystals] == [2, 3, 20, 1, 3, 1, 1, 2, 3]
    dev, g, src = _run(crystals, spoil=[(1, 7, 2, 1), (3, 12, 0, 0)])
    status = [int(d["status"]) for d in dev]
    assert status == [R.OK, R.BAD_INPUT, R.OK, R.BAD_INPUT, R.BAD_INPUT, R.BAD_INPUT, R.OK, R.SINGULAR, R.OK]
    _compare(crystals, dev, g, "bad input")   # (the others against their own references: the bits of a crystal alone)
    for b in (4, 5):
        assert np.isnan(dev[b]["rows"]).all() and (dev[b]["lats"] == 0.0).all()   # the flat lattice was copied as it is
    s = dev[7]
    assert not s["C"].any() and not s["evals"].any() and np.isnan(s["S"]).all() and np.isnan(s["moduli"][1:]).all() and not s["moduli"][0, :2].any()
    assert s["asym"] == 0.0 and int(s["n_negative"]) == 0
    assert torch.equal(src["evals"].view(torch.int64), _sym_eigvals(src).view(torch.int64))   # NaN for NaN as well


def test_relaxation_statuses_reach_the_rows():
    """mi_elastic_collect with an istate: a FAILED copy gives a NaN row (its crystal is BAD_INPUT), an EXHAUSTED one sets the flag (counted
    in n_unrelaxed); CONVERGED and ACTIVE copies are plain rows."""
    crystals = kernel_crystals()[:2] + kernel_crystals()[4:]
    ists = [[R.RELAX_CONVERGED] * R.COPIES for _ in crystals]
    ists[0][3] = ists[0][12] = R.RELAX_EXHAUSTED
    ists[1][9] = R.RELAX_FAILED
    ists[2][5] = 0
    dev, g, _ = _run(crystals, ists=ists, batch_size=7)
    _compare(crystals, dev, g, "istate", ists=ists)
    assert [int(d["status"]) for d in dev] == [R.OK, R.BAD_INPUT, R.OK] and [int(d["n_unrelaxed"]) for d in dev] == [2, -1, 0]
    assert dev[0]["rows"][3, 7] == 1.0 and dev[0]["rows"][4, 7] == 0.0 and np.isnan(dev[1]["rows"][9]).all() and np.isfinite(dev[1]["rows"][8]).all()


def test_a_bad_plan_entry_writes_nothing():
    """A plan entry outside the source, a copy index past 12 or below 0 and an atom count that is not the source crystal's: neither strain
    nor collect writes for them, and nothing is read through the bad index; the good entry beside them is written."""
    from matinvent_amd import _lib, elasticity as EL
    from matinvent_amd.cspnet import _stream
    lib, e = _lib.load(), _e()
    crystals = [kernel_crystals()[1], kernel_crystals()[4]]   # 2 and 3 atoms
    na = [2, 3]
    src = EL.source_arrays(e, (_t(np.concatenate([sp["frac"] for sp in crystals])), _t(np.stack([sp["lat"] for sp in crystals])), torch.zeros(5, 100).cuda()), na)
    src["ws"].fill_(float("nan"))
    src["asym"].fill_(-3.0)
    cna = [2, 3, 2, 3, 2, 3]
    plan_src = np.array([0, 1, -1, 2, 1, 1], np.int32)
    plan_copy = np.array([3, 13, 0, 0, 0, -1], np.int32)   # good | copy 13 | src < 0 | src = Bs | 2 atoms for 3 | copy -1
    cb = e.predictor.make_batch(cna)
    bufs = EL.chunk_buffers(e, len(cna), sum(cna))
    for k in ("types", "frac", "lat"):
        bufs[k].fill_(-7.0)
    bufs["g_lat"].zero_()
    dps, dpc = _t(plan_src), _t(plan_copy)
    args = EL.chunk_args(e, src, dps, dpc, bufs, relaxed=False)
    _lib.check(lib.mi_elastic_strain(cb._h, C.byref(args), _stream()), "mi_elastic_strain")
    _lib.check(lib.mi_elastic_collect(cb._h, C.byref(args), _stream()), "mi_elastic_collect")
    x, l, ty, ws = bufs["frac"].cpu().numpy(), bufs["lat"].cpu().numpy(), bufs["types"].cpu().numpy(), src["ws"].cpu().numpy()
    cb.release()
    assert np.array_equal(x[:2], crystals[0]["frac"]) and np.array_equal(l[0], R.strain(crystals[0]["lat"], 3, H)) and not ty[:2].any()
    assert (x[2:] == -7.0).all() and (l[1:] == -7.0).all() and (ty[2:] == -7.0).all()
    written = np.isfinite(ws)
    assert written[0, 3].all() and not ws[0, 3, :6].any() and ws[0, 3, 6] > 0 and ws[0, 3, 7] == 0.0 and written.sum() == 8
    assert (src["asym"].cpu().numpy() == -3.0).all()   # (no copy 12 in the plan)
    # the C refusals that need a handle
    cb = e.predictor.make_batch([2])
    bufs = EL.chunk_buffers(e, 1, 2)
    args = EL.chunk_args(e, src, dps, dpc, bufs, relaxed=False)
    for field, bad in (("h", 0.0), ("scale", float("inf")), ("det_min", -1.0)):
        keep = getattr(args, field)
        setattr(args, field, bad)
        for fn in (lib.mi_elastic_strain, lib.mi_elastic_collect):
            assert fn(cb._h, C.byref(args), _stream()) == _lib.MI_EINVAL and b"finite and positive" in lib.mi_last_error()
        setattr(args, field, keep)
    args.types = C.c_void_p(bufs["types"].data_ptr() + 4)
    assert lib.mi_elastic_strain(cb._h, C.byref(args), _stream()) == _lib.MI_EINVAL and b"16-byte aligned" in lib.mi_last_error()
    args.types = None
    assert lib.mi_elastic_strain(cb._h, C.byref(args), _stream()) == _lib.MI_EINVAL and b"null argument" in lib.mi_last_error()
    assert lib.mi_elastic_strain(cb._h, None, _stream()) == _lib.MI_EINVAL and b"null argument block" in lib.mi_last_error()
    cb.release()
