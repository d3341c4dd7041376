"""CPU checks of tests/sampler_ref64.py, the float64 yardstick of tests/test_gpu_sampler_arithmetic.py, so that the yardstick is not the
code under test: its step against the reference-generated trajectory fixture (g6) and against oracle.diffcsp_oracle.sample run in
float64 at a network with non-zero heads; the states and the noise it writes (finite on every element, every boundary coordinate
really crossing, the hair-below-zero elements really wrapping); the arithmetic facts of the shapes the GPU file runs; and the GPU
file's whole harness driven on the CPU with step(..., dtype=float32) in the device's place."""
import numpy as np
import pytest
import torch

import tests.test_gpu_sampler_arithmetic as GT
from oracle import diffcsp_oracle as O
from tests import sampler_ref64 as R
from tests.gpu_util import params_from_golden
from tests.kl_util import step_scalars
from tests.traj_util import forward_logprb as oracle_forward_logprb

T = R.T
F32 = 2.0 ** -24          # half an ulp of 1: the unit of the fixture's float32 round-off
T64 = torch.from_numpy


def _circle(a, b):
    d = (a.double() - b.double()).abs()
    return torch.minimum(d, 1 - d)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(1e-300, float(b.double().abs().max()))


def test_the_shapes_reach_what_they_are_chosen_for():
    """Arithmetic facts of the shapes: a later edit of the shapes must not silently lose them."""
    na = GT.LOOP_NA
    assert [3 * n for n in na if 3 * n > 200] == [255, 258, 513]
    assert [-(-3 * n // 256) for n in (85, 86, 171)] == [1, 2, 3] and all(3 * n % 256 for n in (85, 86, 171))     # `idx += 256`: last trip partial
    assert sorted({-(-3 * n // 64) for n in na}) == [1, 4, 5, 9] and all(3 * n % 64 for n in na)                     # `idx += 64`: 1 .. 9 trips, last partial
    assert 3 * 21 < 64 < 3 * 22 and 3 * 85 < 256 < 3 * 86                                                          # second trips from n = 22 and n = 86
    assert {n % 4 for n in na} == {1, 2, 3} and [len(range(w, 86, 4)) for w in range(4)] == [22, 22, 21, 21]      # `i += 4`: unequal trips per wave
    assert len(GT.GRID_NA) == 300 and set(GT.GRID_NA) == {1, 2, 3} and 3 * sum(GT.GRID_NA) > 4 * 256                # several blocks of the wrap kernels
    assert (3 * GT.NODE_OFF) % 4 and (9 * GT.GRAPH_OFF) % 4 and (100 * GT.NODE_OFF) % 4 == 0                        # the draws start inside a Philox quad
    for shape in (na, GT.GRID_NA, GT.HEADS_NA):
        off = np.concatenate([[0], np.cumsum(shape)])
        first, last, hc, hp = R.boundary(shape)
        assert first.tolist() == (3 * off[:-1]).tolist() and last.tolist() == (3 * off[1:] - 1).tolist()
        assert len({hc, hp} | set(first.tolist()) | set(last.tolist())) == 2 * len(shape) + 2
    # every crystal of more than 64 atoms: its last coordinate (a boundary element) lies in the last, partial trip of both loops; the hair
    # elements: local index 511 of the 171-atom crystal (the corrector's ninth trip) and 256 of the 86-atom crystal (the predictor's second)
    first, last, hc, hp = R.boundary(na)
    assert hc - int(first[5]) == 511 and 511 // 64 == 7 and (513 - 1) // 64 == 8 and hp - int(first[3]) == 256 and 256 // 256 == 1


def test_step_reproduces_the_reference_generated_trajectory(golden):
    """step fed the oracle's float32 predictions at the fixture's states and the fixture's noise, against the reference-generated 20-step
    trajectory (g6), teacher-forced at every t = 20 .. 1.  In float64 the states agree within the fixture's own float32 round-off --
    measured: coordinates (x_mid and the next state, on the circle) 1.7e-7 = 2.8 x 2^-24, lattices and logits 1.4e-7 = 2.4 x 2^-24 of
    max|ref|; asserted: 4 x 2^-24.  The fixture's log-probabilities are float32 formulas on float32 states: float64 differs from them by
    the resolution term of DESIGN 21 (reported, not asserted: log_prob_l up to 3.2e-2 absolute at t = 2, where one ulp of the Normal mean is a sizeable part of sigma;
    log_prob_t 4.4e-5, log_prob_x 2.9e-6), which is why the GPU file measures its yardstick instead of fixing one.  step in float32 --
    that yardstick -- reproduces them: measured 0 (bit for bit) on the host this was written on, asserted 1e-5 of max|ref| (libm)."""
    g = golden("g6_sample")
    P = params_from_golden(g)
    Tn, step_lr, na = int(g["T"]), float(g["step_lr"]), T64(g["num_atoms"]).long()
    hp = O.CSPNetHParams(hidden_dim=64, num_layers=2, num_freqs=8)
    beta = {k: P[f"beta_scheduler.{k}"] for k in ("alphas", "alphas_cumprod", "sigmas")}
    sigma = {k: P[f"sigma_scheduler.{k}"] for k in ("sigmas", "sigmas_norm")}
    freqs = T64(g["time_freqs"])
    worst = dict(coords=0.0, state=0.0, lp64=0.0, lp32=0.0)
    for t in range(Tn, 0, -1):
        state = dict(num_atoms=na, **{k: T64(g[f"traj_{t}_{k}"]) for k in GT.STATE_KEYS})
        z = None if t == 1 else {k: T64(g[f"n_{k}_{t}"]) for k in R.NOISE_KEYS}
        tt = torch.full((len(na),), t)
        s = step_scalars(beta, sigma, R.SIGMA_BEGIN, tt, step_lr)
        preds = R.network_preds(hp, P, step_scalars(beta, sigma, R.SIGMA_BEGIN, tt, step_lr, torch.float32), state, z, t, torch.float32, freqs=freqs)
        out = R.step(s, state, preds, z)
        o32 = R.step(step_scalars(beta, sigma, R.SIGMA_BEGIN, tt, step_lr, torch.float32), state, preds, z, dtype=torch.float32)
        assert all(bool(torch.isfinite(v).all()) for v in list(out.values()) + list(o32.values()))
        worst["coords"] = max(worst["coords"], float(_circle(out["frac_coords"], T64(g[f"traj_{t-1}_frac_coords"])).max()))
        for k in ("lattices", "atom_types"):
            worst["state"] = max(worst["state"], _rel(out[k], T64(g[f"traj_{t-1}_{k}"])))
        if t > 1:
            worst["coords"] = max(worst["coords"], float(_circle(out["x_mid"], T64(g[f"traj_{t}_frac_coords_mid"])).max()))
            for k in GT.LP:
                worst["lp64"] = max(worst["lp64"], _rel(out["lp" + k[-2:]], T64(g[f"traj_{t}_{k}"])))
                worst["lp32"] = max(worst["lp32"], _rel(o32["lp" + k[-2:]], T64(g[f"traj_{t}_{k}"])))
    print("g6 teacher-forced, step vs fixture:", worst)
    assert worst["coords"] <= 4 * F32 and worst["state"] <= 4 * F32 and worst["lp32"] <= 1e-5, worst


def _network(seed=5):
    hp = O.CSPNetHParams(hidden_dim=64, num_layers=2, num_freqs=8)
    return hp, O.init_params(hp, seed=seed, head_scale=0.3)


@pytest.mark.parametrize("t,keep", [(2, None), (433, None), (T, None), (1, None), (433, "coords"), (433, "lattice")])
def test_step_matches_the_float64_oracle(t, keep):
    """step fed the oracle's own float64 predictions = oracle.diffcsp_oracle.sample's step in float64, to 1e-12 (coordinates on the
    circle), at a network with non-zero heads, at t = 2, 433, T and t = 1, and in both CSP modes."""
    tabs = R.tables()
    hp, P = _network()
    na = [1, 4, 86, 2]
    s = R.scalars(tabs, t, len(na))
    state = R.build_step_state(na, t, s, seed=3)
    z = None if t == 1 else R.build_noise(na, t, s, seed=4)
    kw = dict(keep_coords=keep == "coords", keep_lattice=keep == "lattice")
    preds = R.network_preds(hp, P, s, state, z, t, torch.float64, keep_coords=kw["keep_coords"])
    assert min(float(v.abs().max()) for v in preds) > 1e-3
    out = R.step(s, state, preds, z, **kw)
    rec, nxt = R.oracle_step(hp, P, tabs, state, z, t, torch.float64, **kw)
    assert float(_circle(out["frac_coords"], nxt["frac_coords"]).max()) <= 1e-12
    assert _rel(out["lattices"], nxt["lattices"]) <= 1e-12 and _rel(out["atom_types"], nxt["atom_types"]) <= 1e-12
    if t > 1:
        assert float(_circle(out["x_mid"], rec["frac_coords_mid"]).max()) <= 1e-12
        for k in GT.LP:
            assert _rel(out["lp" + k[-2:]], rec[k]) <= 1e-12, k
    else:
        assert "lp_x" not in out and "log_prob_x" not in rec
    if keep == "lattice":
        assert torch.equal(out["lattices"], state["lattices"].double())
    if keep == "coords":
        assert torch.equal(out["frac_coords"], state["frac_coords"].double()) and torch.equal(out["x_mid"], out["frac_coords"])


def test_init_state_and_step_noise_are_the_host_philox_contract():
    """init_state / philox_noise on a shard = the slices of oracle.diffcsp_oracle.philox_sampler_noise's draws of the whole batch."""
    na, seed, Tn = torch.tensor([3, 5, 2, 7]), 99, 12
    whole = O.philox_sampler_noise(seed, na, Tn, t_stop=Tn - 1)
    n0, g0 = 8, 2
    x, l, a = R.init_state(seed, Tn, na[g0:].tolist(), node_offset=n0, graph_offset=g0)
    assert torch.equal(x, whole["x_T"][n0:]) and torch.equal(l, whole["l_T"][g0:]) and torch.equal(a, whole["t_T"][n0:])
    z = R.philox_noise(seed, Tn, na[g0:].tolist(), node_offset=n0, graph_offset=g0)
    for k in R.NOISE_KEYS:
        assert torch.equal(z[k], whole[k][Tn][g0 if k == "pred_l" else n0:]), k
    assert float(x.min()) >= 0 and float(x.max()) < 1


@pytest.mark.parametrize("na", [GT.LOOP_NA, GT.GRID_NA, GT.HEADS_NA], ids=["crystal-loop-shapes", "grid-shapes", "non-zero-heads-shapes"])
def test_built_states_cross_the_boundary_and_every_reference_output_is_finite(na):
    """The sets of the GPU test at every t it uses: the reference and the float32 formulas are finite on every element (nothing may be
    left out of a comparison), every boundary coordinate really crosses in both halves of the step, and the hair-below-zero elements
    really wrap: pymod1's 1.0f in the float32 formulas, folded to 0 by the second one."""
    tabs = R.tables()
    B = len(na)
    bias = torch.randn(100, generator=torch.Generator().manual_seed(1))
    preds = R.zero_head_preds(na, bias)
    first, last, hc, hp = R.boundary(na)
    for t in (2, 433, 434, T, 1):
        s, s32 = R.scalars(tabs, t, B), R.scalars(tabs, t, B, torch.float32)
        state = R.build_step_state(na, t, s, seed=17)
        x = state["frac_coords"].view(-1)
        assert state["frac_coords"].dtype == torch.float32 and float(x.min()) == 0 and float(x.max()) == R.LAST_BELOW_ONE
        assert bool((x[first] == 0).all()) and bool((x[last] == R.LAST_BELOW_ONE).all()) and float(x[hc]) == 0 and float(x[hp]) == 0
        z = None if t == 1 else R.build_noise(na, t, s, seed=17 + t)
        o64, o32 = R.step(s, state, preds, z), R.step(s32, state, preds, z, dtype=torch.float32)
        for o in (o64, o32):
            assert all(bool(torch.isfinite(v).all()) for v in o.values())
            assert float(o["frac_coords"].min()) >= 0 and float(o["frac_coords"].max()) < 1
        if t == 1:
            assert torch.equal(o64["frac_coords"], state["frac_coords"].double()) and "lp_x" not in o64
            continue
        for k in ("corr_x", "pred_x"):
            zz = z[k].view(-1)
            assert float(zz[first].max()) <= -0.5 and float(zz[first].min()) >= -3 and float(zz[last].min()) >= 0.5 and float(zz[last].max()) <= 3
        for k in ("x_mid_raw", "frac_raw"):
            v = o64[k].view(-1)
            assert float(v[first].max()) < 0 and float(v[last].min()) >= 1, (t, k)                 # every boundary coordinate crosses
        assert -2 * R.HAIR < float(o64["x_mid_raw"].view(-1)[hc]) < 0 and float(o32["x_mid"].view(-1)[hc]) == 1.0
        assert float(o64["x_mid_raw"].view(-1)[hp]) == 0 and -2 * R.HAIR < float(o64["frac_raw"].view(-1)[hp]) < 0
        assert float((o32["frac_raw"] % 1.0).view(-1)[hp]) == 1.0 and float(o32["frac_coords"].view(-1)[hp]) == 0.0
        for k in ("lp_l", "lp_t", "lp_x"):
            assert _rel(o32[k], o64[k]) < 1e-3, (t, k)


# ---- the GPU file's harness on the CPU ----------------------------------------------------------------------------------------------------

class Float32StandIn:
    """step(..., dtype=float32) -- for the network with heads the oracle in float32 -- in the device's place, behind the interface of
    test_gpu_sampler_arithmetic.Device: every case, every comparison and the Philox bound of the GPU file run without a GPU."""

    def __init__(self):
        self.nets = {k: GT.TA._params(2, **kw) for k, kw in GT.NETS.items()}
        self.bias = self.nets["zero"][1]["decoder.type_out.bias"]
        self.cache = {}
        self.tables = R.tables()

    def sample(self, net, na, t_start, t_stop, init=None, z=None, seed=GT.SEED, record=True, streams=1, node_offset=0, graph_offset=0, keep=None):
        B, N = len(na), sum(na)
        x, l, a = init if init is not None else R.init_state(seed, T, na, node_offset, graph_offset)
        state = dict(frac_coords=x % 1.0, lattices=l.clone(), atom_types=a.clone(), num_atoms=torch.tensor(na))
        traj = {t_start: dict(state)}
        kw = dict(keep_coords=keep == "coords", keep_lattice=keep == "lattice")
        for t in range(t_start, t_stop, -1):
            zt = None if t == 1 else (z[t] if z is not None else R.philox_noise(seed, t, na, node_offset, graph_offset))
            if net == "zero":
                o = R.step(R.scalars(self.tables, t, B, torch.float32), state, R.zero_head_preds(na, self.bias), zt, dtype=torch.float32, **kw)
                nxt = {k: o[k] for k in GT.STATE_KEYS}
                rec = {} if zt is None else dict(frac_coords_mid=o["x_mid"], log_prob_l=o["lp_l"], log_prob_t=o["lp_t"], log_prob_x=o["lp_x"])
            else:
                rec, nxt = R.oracle_step(*self.nets[net], self.tables, state, zt, t, torch.float32, **kw)
                rec = {k: rec[k] for k in GT.LP + ("frac_coords_mid",) if k in rec}
            traj[t].update(rec)
            state = dict(nxt, num_atoms=state["num_atoms"])
            traj[t - 1] = dict(state)
        zero = dict(frac_coords_mid=torch.zeros(N, 3), **{k: torch.zeros(B) for k in GT.LP})
        rows = {k: traj[t_start].get(k, zero[k]) for k in zero} if record else None
        return traj[t_stop], traj, rows

    def forward_logprb(self, net, state):
        hp, P = self.nets[net]
        return list(oracle_forward_logprb(P, hp, *self.tables, R.SIGMA_BEGIN, state, R.STEP_LR)[:3])


@pytest.fixture(scope="module")
def standin():
    return Float32StandIn()


@pytest.mark.parametrize("shape,t", [("loop", 2), ("loop", 433), ("loop", T), ("grid", 433)])
def test_harness_injected_noise(standin, shape, t):
    GT.run_injected(standin, shape, t)


def test_harness_t1(standin):
    GT.run_t1(standin)


def test_harness_device_noise_and_the_philox_bound(standin):
    GT.run_device_noise(standin)
    GT.run_init_state(standin)


@pytest.mark.parametrize("noise", ["injected", "device"])
def test_harness_record_vs_not(standin, noise):
    GT.run_record_vs_not(standin, noise)


def test_harness_streams(standin):
    GT.run_streams(standin)


@pytest.mark.parametrize("mode", ["coords", "lattice"])
def test_harness_csp(standin, mode):
    GT.run_csp(standin, mode)


@pytest.mark.parametrize("t", GT.TIMES)
def test_harness_nonzero_heads(standin, t):
    GT.run_heads(standin, t)
