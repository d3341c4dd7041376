"""GPU checks of the relaxation on a learned energy (matinvent_amd/csrc/relax.hip under include/matinvent_hip_relax.h; matinvent_amd.relax;
DESIGN 45) against tests/relax_ref64.py.

(1) The step kernel against float64 with the network taken out: gradients of a synthetic harmonic energy (tests/relax_ref64.harmonic), 40
consecutive steps with and without relax_cell on crystals of [1, 2, 171, 20, 3] atoms and on 300 crystals of 1-3 atoms.  Bound, per array:
4 x the float32 host restatement's own deviation from float64 on the same inputs; the decisions (status, positive-
power count, steps) agree exactly -- tests/test_relax_host.py asserts on the CPU that no decision of these runs is tied.  (2) mi_relax_run
against mi_relax_init + a loop of the public pieces, bit for bit.  (3) Freezing.  (4) The energy falls along the first step.
(5) relax_records.  (6) The pipelines.  Nothing is claimed about the quality of a relaxed structure: no weight here is trained."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import diffcsp_oracle as O
from tests import input_grad_ref as IR
from tests import relax_ref64 as R
from tests import scalar_ref as SR
from tests.test_relax_host import CASES, STEPS, TEST_PARAMS

pytestmark = pytest.mark.gpu

BOUND = 4.0       # x the float32 restatement's own deviation from float64
GRAD_TOL = 2e-5   # of max|ref|: the input gradient's own bound (tests/test_gpu_input_grad.py)


def _lib_():
    from matinvent_amd import _lib
    return _lib, _lib.load()


def _cparams(prm):
    from matinvent_amd import _lib
    return _lib.RelaxParams(*[prm[k] for k in R.FLOATS], int(prm["n_min"]), int(prm["relax_cell"]), int(prm["per_atom"]))


@functools.lru_cache(maxsize=None)
def _plain_model():
    """A predictor whose handles the synthetic-gradient tests run on (mi_relax_step reads the handle's offsets alone)."""
    from matinvent_amd import predictor as PR
    return PR.PropertyPredictor(["energy"], hidden_dim=64, num_layers=2, time_dim=256, num_freqs=8, ln=True, device="cuda", seed=3)


@functools.lru_cache(maxsize=None)
def _references(name, cell):
    """The float64 reference and the float32 restatement of a case: computed once, shared, left unchanged."""
    na, seed = CASES[name]
    case = R.make_case(na, seed)
    prm = R.params(relax_cell=cell, **TEST_PARAMS)
    s64, r64 = R.run(case, prm, STEPS, np.float64)
    s32, _ = R.run(case, prm, STEPS, np.float32)
    return case, prm, s64, s32, R.branch_report(case, r64, s64)


def _device_run(case, prm, steps):
    """tests/relax_ref64.run with mi_relax_step in fire_step's place: the state lives on the device, every step's gradients come from
    `harmonic` at the device's own state (float64 from its float32 arrays, rounded to float32)."""
    from matinvent_amd.cspnet import _ptr, _stream
    _lib, lib = _lib_()
    na = case["na"]
    B, N = len(na), sum(na)
    cb = _plain_model().make_batch(na)
    cp = _cparams(prm)
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    x, l = t(case["frac"]), t(case["lat"])
    vx, vl, fs = torch.empty(N, 3, device="cuda"), torch.empty(B, 3, 3, device="cuda"), torch.empty(B, R.NF, device="cuda")
    is_, d_out = torch.empty(B, R.NI, dtype=torch.int32, device="cuda"), torch.empty(B, 1, device="cuda")
    _lib.check(lib.mi_relax_init(cb._h, C.byref(cp), 1, 0, _ptr(vx), _ptr(vl), _ptr(fs), _ptr(is_), _ptr(d_out), _stream()), "mi_relax_init")
    assert bool((d_out == 1).all()) and not vx.any() and not vl.any() and not is_.any()
    assert torch.equal(fs.cpu(), torch.tensor([prm["dt"], prm["a_start"], 0, 0, 0, 0], dtype=torch.float32).repeat(B, 1))
    for _ in range(steps):
        E, gx, gl = R.harmonic(na, case["spec"], x.cpu().numpy(), l.cpu().numpy())
        g_frac, g_lat, out = t(gx.astype(np.float32)), t(gl.astype(np.float32)), t(E.astype(np.float32)).view(B, 1)   # (named: alive over the call)
        _lib.check(lib.mi_relax_step(cb._h, C.byref(cp), 1, 0, _ptr(x), _ptr(l), _ptr(vx), _ptr(vl), _ptr(fs), _ptr(is_), _ptr(g_frac), _ptr(g_lat), _ptr(out),
                                     _stream()), "mi_relax_step")
    st = dict(frac=x.cpu().numpy(), lat=l.cpu().numpy(), vel_x=vx.cpu().numpy(), vel_l=vl.cpu().numpy(), fs=fs.cpu().numpy(), is_=is_.cpu().numpy())
    cb.release()
    return st


@pytest.mark.parametrize("name", ["loop", "grid"])
@pytest.mark.parametrize("cell", [0, 1])
def test_step_kernel_vs_float64_over_consecutive_steps(name, cell):
    """Measured on the device (MI_TOL_REPORT prints the figures): DESIGN 45."""
    case, prm, s64, s32, rep = _references(name, cell)
    # the reference run is what the issue demands of it (asserted on the CPU too: tests/test_relax_host.py)
    assert min(rep["m_P"], rep["m_fmax"], rep["m_clamp"]) > R.TIE and rep["nonpositive"] and rep["grew"] and rep["converged_mid_run"] and rep["one_atom_at_step_0"], rep
    if name == "loop":
        assert rep["capped"] and rep["clamped"] and max(case["na"]) == 171 and min(case["na"]) == 1
    else:
        assert len(case["na"]) == 300 and set(case["na"]) == {1, 2, 3}
    dev = _device_run(case, prm, STEPS)
    own, err = R.deviation(s32, s64), R.deviation(dev, s64)
    bad = []
    for k in own:
        if k == "is_equal":
            continue
        if os.environ.get("MI_TOL_REPORT"):
            print(f"TOL relax {name} cell={cell} {k}: device vs float64 {err[k]:.3e}; float32 restatement vs float64 {own[k]:.3e}; "
                  f"ratio {err[k] / own[k] if own[k] > 0 else (0.0 if err[k] == 0 else float('inf')):.2f} (demanded <= {BOUND:g})")
        if not (np.isfinite(err[k]) and err[k] <= BOUND * own[k]):
            bad.append(f"{k}: device {err[k]:.3e} > {BOUND:g} x {own[k]:.3e}")
    assert err["is_equal"], f"{name} cell={cell}: the device took another decision than float64:\n{dev['is_'][(dev['is_'] != s64['is_']).any(axis=1)]}"
    assert not bad, f"{name} cell={cell}: " + "; ".join(bad)
    # no crystal was excluded, and the one-atom crystals converged at step 0 without moving
    one = np.asarray(case["na"]) == 1
    assert (dev["is_"][one, R.I_STATUS] == R.CONVERGED).all() and not dev["is_"][one, R.I_STEPS].any()
    if not cell:
        assert np.array_equal(dev["lat"], case["lat"]) and not dev["vel_l"].any()


# ---- on the reference fixture's weights ---------------------------------------------------------------------------------------------------

_G15 = {}


def _g15_case(golden):
    """g15's predictor, its three crystals as a clean state, and the float32 oracle (tests/scalar_ref.forward + autograd)."""
    if "c" not in _G15:
        from tests.test_gpu_scalar import _g15
        m, P, fs = _g15(golden)
        na = fs["num_atoms"]
        B = len(na)
        _, onehot, fr, lat = SR.clean_inputs(fs["atom_types"], fs["frac"], fs["lengths"], fs["angles"], torch.zeros(B), 256, torch.float32)
        _G15["c"] = dict(m=m, P=P, na=na, types=onehot.contiguous(), frac=fr.contiguous(), lat=lat.contiguous(),
                         hp=O.CSPNetHParams(hidden_dim=64, num_layers=2, num_freqs=8), temb=O.time_embedding(torch.zeros(B).long(), 256).float())
    return _G15["c"]


def _state(c):
    return (c["frac"].cuda(), c["lat"].cuda(), c["types"].cuda())


# dt = 4 (2 after the first step's halving): on these weights the forces are ~1e-2, so the first move is ~0.2 A and the oracle's energy falls
# by 3e-4 .. 1e-2 -- three orders above float32's resolution of an output of size 1 (picked on the CPU oracle alone)
G15_FIRE = dict(dt=4.0, dt_max=8.0, maxstep=1.0, fmax=1e-9, per_atom=False)


def test_relax_run_equals_init_and_a_loop_of_the_public_pieces(golden):
    from matinvent_amd import predictor as PR, relax as RX
    from matinvent_amd.cspnet import _ptr, _stream
    _lib, lib = _lib_()
    c = _g15_case(golden)
    m, na = c["m"], c["na"].tolist()
    for cell in (True, False):
        r = RX.Relaxer(m, "y", steps=10, relax_cell=cell, **G15_FIRE)
        cb = m.make_batch(na)
        a = _state(c)
        bufs = RX.relax_enqueue(r, a, cb)
        # the same with the public pieces: the clean predictor's input gradient through the C entry (predictor.input_gradient asks for a noised one)
        b = _state(c)
        w = RX.relax_buffers(r, len(na), sum(na), m.device)
        prm = r.params()
        _, W, bias = m.head_slices()
        _lib.check(lib.mi_relax_init(cb._h, C.byref(prm), 1, 0, _ptr(w["vel_x"]), _ptr(w["vel_l"]), _ptr(w["fs"]), _ptr(w["is_"]), _ptr(w["d_out"]), _stream()))
        for _ in range(10):
            _lib.check(lib.mi_scalar_input_grad(m.trunk._h, cb._h, _ptr(b[2]), _ptr(b[0]), _ptr(b[1]), _ptr(m.time_freqs), None, 0, _ptr(W), _ptr(bias), 1,
                                                _ptr(w["d_out"]), _ptr(w["out"]), None, _ptr(w["g_frac"]), _ptr(w["g_lat"]), _stream()))
            _lib.check(lib.mi_relax_step(cb._h, C.byref(prm), 1, 0, _ptr(b[0]), _ptr(b[1]), _ptr(w["vel_x"]), _ptr(w["vel_l"]), _ptr(w["fs"]), _ptr(w["is_"]),
                                         _ptr(w["g_frac"]), _ptr(w["g_lat"]), _ptr(w["out"]), _stream()))
        # still ACTIVE: the run's last launch marks them (a one-atom crystal with a fixed cell has no force at all: CONVERGED at step 0)
        assert w["is_"][:, 0].tolist() == [_lib.RELAX_CONVERGED if (n == 1 and not cell) else _lib.RELAX_ACTIVE for n in na]
        assert bufs["is_"][:, 0].tolist() == [_lib.RELAX_CONVERGED if (n == 1 and not cell) else _lib.RELAX_EXHAUSTED for n in na]
        assert torch.equal(bufs["is_"][:, 1:], w["is_"][:, 1:]) and bufs["is_"][:, 2].tolist() == [0 if (n == 1 and not cell) else 10 for n in na]
        for k in ("vel_x", "vel_l", "fs", "out", "g_frac", "g_lat"):
            assert torch.equal(bufs[k], w[k]), k
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], c["types"].cuda())
        assert not torch.equal(a[0], c["frac"].cuda()) and (not cell) == torch.equal(a[1], c["lat"].cuda())
        # check_every reads the active count and changes nothing else
        r2 = RX.Relaxer(m, "y", steps=10, relax_cell=cell, check_every=4, **G15_FIRE)
        d = _state(c)
        bufs2 = RX.relax_enqueue(r2, d, cb)
        assert torch.equal(d[0], a[0]) and torch.equal(d[1], a[1]) and torch.equal(bufs2["is_"], bufs["is_"]) and torch.equal(bufs2["fs"], bufs["fs"])
        cb.release()


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def test_freezing(golden):
    from matinvent_amd import relax as RX
    from matinvent_amd.cspnet import _ptr, _stream
    _lib, lib = _lib_()
    c = _g15_case(golden)
    m, na = c["m"], c["na"].tolist()
    off = np.concatenate([[0], np.cumsum(na)])
    cb = m.make_batch(na)
    # fmax huge: every crystal CONVERGED at step 0, the state bit-unchanged (coordinates outside [0, 1) are not even re-wrapped)
    x0 = c["frac"].clone()
    x0[1, 0] += 1.0
    st = (x0.cuda(), c["lat"].cuda(), c["types"].cuda())
    out, info = RX.relax_state(RX.Relaxer(m, "y", steps=5, **dict(G15_FIRE, fmax=1e9)), st, cb)
    assert info["status"].tolist() == [_lib.RELAX_CONVERGED] * 3 and not info["steps"].any() and info["status_names"][0] == "converged"
    assert torch.equal(_bits(out[0]), _bits(st[0])) and torch.equal(_bits(out[1]), _bits(st[1]))
    assert np.array_equal(info["e_first"], info["e_last"]) and np.isfinite(info["e_last"]).all() and (info["fmax"] > 0).all()
    # a non-finite coordinate: that crystal FAILED and bit-unchanged, its neighbours move as they do without it
    r = RX.Relaxer(m, "y", steps=1, **G15_FIRE)
    good, ginfo = RX.relax_state(r, _state(c), cb)
    xb = c["frac"].clone()
    xb[off[1] + 2, 1] = float("nan")
    stb = (xb.cuda(), c["lat"].cuda(), c["types"].cuda())
    badr, binfo = RX.relax_state(r, stb, cb)
    _lib.saturation_events(reset=True)   # (the NaN went through the network's operand conversions, which count it process-wide: not this file's to leave behind)
    assert binfo["status"].tolist() == [_lib.RELAX_EXHAUSTED, _lib.RELAX_FAILED, _lib.RELAX_EXHAUSTED] and binfo["steps"].tolist() == [1, 0, 1]
    assert np.isnan(binfo["e_last"][1]) and np.isfinite(binfo["e_last"][[0, 2]]).all()
    rows = slice(off[1], off[2])
    assert torch.equal(_bits(badr[0][rows]), _bits(stb[0][rows])) and torch.equal(_bits(badr[1][1]), _bits(stb[1][1]))
    for b in (0, 2):   # the move is dt^2 F: a gradient within GRAD_TOL of its largest element moves the state within GRAD_TOL of its largest move (+ the wrap's rounding)
        rb = slice(off[b], off[b + 1])
        for k, start in ((0, c["frac"][rb]), (1, c["lat"][b])):
            g, w_, s0 = good[k][rb if k == 0 else b].cpu().double(), badr[k][rb if k == 0 else b].cpu().double(), start.double()
            move = (g - s0).abs().max()
            assert (float(move) > 0 or (k == 0 and na[b] == 1)) and float((g - w_).abs().max()) <= GRAD_TOL * float(move) + 2.4e-7, \
                (b, k, float((g - w_).abs().max()), float(move))   # (a lone atom feels no force: only its cell moves)
    # steps = 0 and B = 0 launch nothing: the arrays keep a pattern
    r0 = RX.Relaxer(m, "y", steps=0, **G15_FIRE)
    s0 = _state(c)
    bufs = RX.relax_buffers(r0, len(na), sum(na), m.device)
    for k in ("out", "g_frac", "g_lat"):
        bufs[k].fill_(7.0)
    RX.relax_enqueue(r0, s0, cb, bufs=bufs)
    assert all(bool((bufs[k] == 7.0).all()) for k in ("out", "g_frac", "g_lat")) and not bufs["is_"].any() and torch.equal(s0[0], c["frac"].cuda())
    info0 = RX.read_info(r0, bufs, na)
    assert info0["status"].tolist() == [_lib.RELAX_ACTIVE] * 3 and np.isnan(info0["e_last"]).all()
    e = m.make_batch([])
    prm = r0.params()
    assert lib.mi_relax_init(e._h, C.byref(prm), 1, 0, *([None] * 5), _stream()) == 0
    assert lib.mi_relax_step(e._h, C.byref(prm), 1, 0, *([None] * 9), _stream()) == 0
    assert lib.mi_relax_run(m.trunk._h, e._h, C.byref(prm), *([None] * 6), 1, 0, *([None] * 8), 5, 1, _stream()) == 0
    # refusals, by name, before anything is enqueued
    for kw, text in ((dict(steps=-1), "steps = -1"), (dict(p=1), "property p = 1 of P = 1")):
        rc = lib.mi_relax_run(m.trunk._h, cb._h, C.byref(prm), _ptr(s0[2]), _ptr(s0[0]), _ptr(s0[1]), _ptr(m.time_freqs), None, None, 1, kw.get("p", 0),
                              *([None] * 8), kw.get("steps", 1), 1, _stream())
        assert rc == _lib.MI_EINVAL and text in lib.mi_last_error().decode(), lib.mi_last_error()
    bad = r0.params()
    bad.fmax = float("nan")
    assert lib.mi_relax_step(cb._h, C.byref(bad), 1, 0, *([None] * 9), _stream()) == _lib.MI_EINVAL and b"fmax" in lib.mi_last_error()
    torch.cuda.synchronize()
    assert all(bool((bufs[k] == 7.0).all()) for k in ("out", "g_frac", "g_lat"))
    e.release()
    cb.release()


def test_the_energy_falls_along_the_first_step(golden):
    """From v = 0 the first move is straight along the force (P = 0: dt halves, dr = dt^2 F).  The device's own energy falls for every
    crystal, and so does the float32 oracle's under its own gradient and the reference step."""
    from matinvent_amd import predictor as PR, relax as RX
    c = _g15_case(golden)
    m, na = c["m"], c["na"].tolist()
    cb = m.make_batch(na)
    r = RX.Relaxer(m, "y", steps=1, relax_cell=True, **G15_FIRE)
    st = _state(c)
    e0 = PR.forward_state(m, st, cb, 0).cpu()[:, 0]
    out, info = RX.relax_state(r, st, cb)
    e1 = PR.forward_state(m, out, cb, 0).cpu()[:, 0]
    assert info["steps"].tolist() == [1, 1, 1] and np.allclose(info["dt"], 2.0) and bool((e1 < e0).all()), (e0, e1)
    assert np.allclose(info["e_first"], e0.double().numpy(), rtol=0, atol=GRAD_TOL)   # (the taped forward against the inference form: DESIGN 43's bound)
    # the oracle: float32 autograd of tests/scalar_ref.forward, the reference's step at float32, the oracle's energy again
    d_out = torch.ones(len(na), 1)
    o0, gx, gl, _ = IR.input_grad(c["P"], c["hp"], c["temb"], c["types"], c["frac"], c["lat"], c["na"], d_out, torch.float32)
    prm = R.params(relax_cell=1, **G15_FIRE)
    ref = R.new_state(na, c["frac"].numpy(), c["lat"].numpy(), prm, np.float32)
    rec = R.fire_step(na, prm, ref, gx.numpy(), gl.numpy(), o0.reshape(-1).numpy())
    o1, _, _ = SR.forward(c["P"], c["hp"], c["temb"], c["types"], torch.from_numpy(ref["frac"]), torch.from_numpy(ref["lat"]), c["na"], torch.float32)
    assert rec["moved"].all() and not rec["positive"].any() and bool((o1.reshape(-1) < o0.reshape(-1)).all()), (o0, o1)
    # and the device's step is the oracle's: the move dt^2 F within the gradient's bound
    for k, dev, start in (("frac", out[0], c["frac"]), ("lat", out[1], c["lat"])):
        d = np.abs(dev.cpu().double().numpy() - ref[k].astype(np.float64))
        d = np.minimum(d, 1 - d) if k == "frac" else d
        move = np.abs(ref[k].astype(np.float64) - start.double().numpy()).max()
        assert move > 1e-3 and d.max() <= GRAD_TOL * move + 2.4e-7, (k, d.max(), move)
    cb.release()


def test_relax_records_round_trip(golden):
    from matinvent_amd import relax as RX
    from matinvent_amd.data import SimpleStructure
    from matinvent_amd.structure import lattice_matrix
    c = _g15_case(golden)
    rng = np.random.default_rng(4)
    recs = []
    for n in (3, 1, 5, 2, 4):
        recs.append(SimpleStructure((4.0 + 2.0 * rng.random(3)).tolist(), (80.0 + 20.0 * rng.random(3)).tolist(), rng.integers(1, 90, n).tolist(), rng.random((n, 3))))
    recs.insert(2, SimpleStructure([4.0, 4.0, 4.0], [90.0, 90.0, 90.0], [150], np.zeros((1, 3))))       # not a crystal the network takes
    recs.insert(4, SimpleStructure([4.0, 4.0, 4.0], [90.0, 90.0, 0.0], [3, 4], rng.random((2, 3))))     # a flat cell: det L = 0, FAILED on the device
    r = RX.Relaxer(c["m"], "y", steps=3, batch_size=4, **G15_FIRE)
    out, e = r(recs, None)
    assert len(out) == len(recs) == 7 and e.shape == (7,) and e.dtype == np.float64
    assert out[2] is recs[2] and out[4] is recs[4] and np.isnan(e[[2, 4]]).all() and np.isfinite(np.delete(e, [2, 4])).all()
    assert r.last_info["status"].tolist() == [3, 3, -1, 3, 2, 3, 3] and r.last_info["steps"].tolist() == [3, 3, 0, 3, 0, 3, 3]
    for i in (0, 1, 3, 5, 6):
        assert out[i].species == recs[i].species and out[i].frac_coords.shape == recs[i].frac_coords.shape and out[i] is not recs[i]
        assert (out[i].frac_coords >= 0).all() and (out[i].frac_coords <= 1).all() and not np.allclose(out[i].lengths, recs[i].lengths, rtol=0, atol=1e-6)
    # lengths / angles reproduce the relaxed matrix's Gram matrix: relax the first four on a handle of our own and compare
    idx = [0, 1, 3, 5]
    na = [len(recs[i].species) for i in idx]
    cb = c["m"].make_batch(na)
    types = torch.zeros(sum(na), 100)
    types[torch.arange(sum(na)), torch.tensor(sum((recs[i].species for i in idx), [])) - 1] = 1.0
    lat = torch.from_numpy(np.stack([lattice_matrix(recs[i].lengths, recs[i].angles) for i in idx])).float()
    frac = torch.from_numpy(np.concatenate([recs[i].frac_coords for i in idx]) % 1.0).float()
    st, info = RX.relax_state(r, (frac.cuda(), lat.cuda(), types.cuda()), cb)
    L = st[1].cpu().double().numpy()
    for k, i in enumerate(idx):
        G = L[k] @ L[k].T
        G2 = lattice_matrix(out[i].lengths, out[i].angles)
        assert np.allclose(G2 @ G2.T, G, rtol=1e-9, atol=1e-9), i
        assert e[i] == info["e_last"][k]
    cb.release()
    logs = RX.log_metrics(r, e)
    assert logs["relax_failed"] == 2 and logs["relax_converged"] == 0 and logs["relax_steps_mean"] == 3 * 5 / 6 and logs["relax_de_mean"] < 0


# ---- the pipelines ------------------------------------------------------------------------------------------------------------------------

LOG_KEYS = ("relax_converged", "relax_failed", "relax_steps_mean", "relax_de_mean")


def _save_energy_predictor(tmp_path):
    from matinvent_amd import predictor as PR
    m = PR.PropertyPredictor(["energy"], hidden_dim=64, num_layers=2, time_dim=256, num_freqs=8, ln=True, device="cuda", seed=5)
    return PR.save_predictor(m, str(tmp_path / "energy_model"))


@pytest.mark.parametrize("how", ["mat_invent", "dropin"])
def test_a_loop_relaxes_before_the_filter_and_the_reward(tmp_path, monkeypatch, how):
    """One MatInvent loop with a Relaxer as sample_cfg.mlip_opt -- built in Python, and composed from configs/relax/surrogate.yaml through
    the drop-in's main: the filter receives energies of the kept length, the reward sees the relaxed structures, the log has the four keys."""
    import csv
    from matinvent_amd import relax as RX
    from matinvent_amd.data import data2struc
    from matinvent_amd.rewards import SyntheticReward
    from matinvent_amd.sampling import DiffCSPSampler
    from tests.test_gpu_fingerprint import FT, _dense, _dropin
    real_gen = DiffCSPSampler.generate

    def gen(self, *a, **kw):   # (the untrained chain's cells are thousands of A wide: give them physical volumes, tests/test_gpu_fingerprint.py)
        data, _ = real_gen(self, *a, **kw)
        data = [_dense(d) for d in data]
        return data, [data2struc(d) for d in data]

    monkeypatch.setattr(DiffCSPSampler, "generate", gen)
    seen = {}
    real_call = RX.Relaxer.__call__

    def call(self, strucs, xyz_path=None):
        out, e = real_call(self, strucs, xyz_path)
        seen.update(given=list(strucs), relaxed=list(out), energies=np.array(e), xyz=xyz_path, exists=bool(xyz_path and os.path.exists(xyz_path)))
        return out, e

    monkeypatch.setattr(RX.Relaxer, "__call__", call)
    real_scoring = SyntheticReward.scoring

    def scoring(self, samples, label="tmp"):
        seen["scored"] = list(samples[0] if isinstance(samples, tuple) else samples)
        return real_scoring(self, samples, label)

    monkeypatch.setattr(SyntheticReward, "scoring", scoring)

    def flt(data, strucs, energies):
        seen.update(flt_n=(len(data), len(strucs), None if energies is None else len(energies)), flt_strucs=list(strucs))
        return data, strucs, {"kept": float(len(strucs))}

    model_dir = _save_energy_predictor(tmp_path)
    if how == "dropin":
        args = ["expname=relax", "+relax@sample_cfg.mlip_opt=surrogate", f"sample_cfg.mlip_opt.model_path={model_dir}", "sample_cfg.mlip_opt.steps=3",
                "sample_cfg.mlip_opt.fmax=1e-9"] + FT
        rl = _dropin(tmp_path, args, 1)
        assert isinstance(rl.sample_cfg.mlip_opt, RX.Relaxer) and rl.sample_cfg.mlip_opt.steps == 3
        rows = list(csv.DictReader(open(tmp_path / "exp_res" / "relax" / "metrics.csv")))
        assert len(rows) == 1
        for k in LOG_KEYS:
            assert k in rows[0] and np.isfinite(float(rows[0][k])), k
        assert float(rows[0]["relax_steps_mean"]) == 3.0 and float(rows[0]["relax_failed"]) == 0.0
    else:
        from matinvent_amd import pipeline
        from matinvent_amd.predictor import load_predictor
        from matinvent_amd.suite import DiffCSPSuite
        suite = DiffCSPSuite("diffcsp", {"batch_size": 4, "num_batches": 1}, {"batch_size": 4, "timesteps": 6, "lr": 1e-4}, device="cuda:0", random_init=True,
                             seed=0, head_scale=0.1, hparams=dict(decoder=dict(hidden_dim=64, num_layers=2, num_freqs=8), beta_scheduler=dict(timesteps=20),
                                                                  sigma_scheduler=dict(timesteps=20)))
        relaxer = RX.Relaxer(load_predictor(model_dir, device="cuda"), "energy", steps=3, fmax=1e-9)
        logged = []

        class Log:
            def log(self, d, step=None):
                logged.append(dict(d))

        rl = pipeline.MatInvent(rl_epoch=1, model_suite=suite, reward=SyntheticReward(), sample_cfg={"mlip_opt": relaxer, "filter": flt, "geometric_filter": False,
                                                                                                  "sample_steps": 5},
                                finetune_cfg={"batch_size": 4, "accum_steps": 3, "epochs": 1, "sigma": 0.025}, topk_ratio=0.5, save_dir=str(tmp_path), save_freq=10,
                                device="cuda:0", logger=Log())
        rl.run_rl()
        assert len(logged) == 1 and all(k in logged[0] for k in LOG_KEYS) and logged[0]["kept"] == 4.0 and logged[0]["relax_steps_mean"] == 3.0
        assert seen["flt_n"] == (4, 4, 4) and all(a is b for a, b in zip(seen["flt_strucs"], seen["relaxed"]))
    assert len(seen["given"]) == len(seen["relaxed"]) == len(seen["energies"]) == 4 and np.isfinite(seen["energies"]).all()
    assert seen["xyz"].endswith("step_0000_valid.extxyz") and seen["exists"]
    assert all(a is b for a, b in zip(seen["scored"], seen["relaxed"])) and all(a is not b for a, b in zip(seen["given"], seen["relaxed"]))
