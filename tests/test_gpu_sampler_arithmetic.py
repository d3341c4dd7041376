"""GPU checks of the reverse sampler's own kernels (matinvent_amd/csrc/sampler.hip: corrector_kernel, predictor_kernel,
mi_sampler_init_state, the two wrap kernels) against the float64 reference tests/sampler_ref64.py, with the network taken out of the
comparison and at the sizes the kernels loop over.

With the agent's three head weight matrices zero the device's predictions are exactly pred_x = 0, pred_l = 0, pred_t = type_out.bias at
any state, so one reverse step is a closed form of the state, the noise and the bias: sampler_ref64.step.  Every case is a single step
(t_start = t, t_stop = t - 1) from an injected state with record=True unless it says otherwise.

Network and schedule: H = 64, L = 2, F = 8, built once per module; the T = 1000 cosine schedule with the packaged sigmas_norm table, so
the step scalars are the workload's (c0 = 100 at t = T, std_pred = 4.8e-4 at t = 2).
Atom counts: LOOP_NA = [1, 2, 85, 86, 3, 171] -- 3n = 255, 258, 513: one, two and three trips of the predictor's `idx += 256`, the last
one partial, 1 to 9 trips of the corrector's `idx += 64`, up to 43 trips of the four-wave type loop `i += 4` with unequal trips per wave
(n = 86: waves 0, 1 take 22 atoms, waves 2, 3 take 21; n mod 4 covers 1, 2, 3).  GRID_NA = 300 crystals of 1..3 atoms: record rows
t * B at B = 300 and several blocks of the wrap kernels.  HEADS_NA = [86, 3, 1] with heads x 0.1: the only case where c1 pl,
step sqrt(sn) px and pymod1(drift) with drift != x reach a later loop trip.
The states (sampler_ref64.build_step_state / build_noise): every crystal's first coordinate is exactly 0 and its last one exactly
nextafter(1, 0), with corrector and predictor draws of the crossing sign; two more coordinates are a hair (1e-9) below 0 after the
corrector and after the predictor -- where pymod1 returns 1.0f and the predictor's second pymod1 must fold it to 0.

Tolerances (measured in the test; DESIGN 25's rule): the yardstick of a quantity is the deviation of step(..., dtype=float32) on the CPU
from float64, relative to max|ref64|; the device gets 4 times that, at least 4 * 2^-24.  Coordinates are compared on the circle, scale 1.
The non-zero-heads case takes the oracle in float32 against the oracle in float64 as its yardstick, capped at what
tests/test_gpu_sampler.py::test_teacher_forced_single_steps demands (1e-5 wrapped, 1e-5 of max|ref|, 1e-4 log-probabilities).  Where the
device draws its own noise the reference is fed the host Philox contract's draws, and a quantity also gets 5e-6 (the project's atol on
the draws) times the sum of the reference's absolute first derivatives with respect to them (float64 autograd of step).
MI_TOL_REPORT=1 prints yardstick, device error and tolerance.

Every test body is a `run_*` function of a `dev` object (Device below: the library); tests/test_sampler_ref64_host.py drives the same
functions on the CPU with step(..., dtype=float32) in the device's place."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tests.test_gpu_traj_arithmetic as TA
from tests import sampler_ref64 as R
from tests.test_gpu_ft_arithmetic import GRAPH_OFF, NODE_OFF, PHILOX_ATOL, _all, _first_order

pytestmark = pytest.mark.gpu

T = R.T
LOOP_NA = [1, 2, 85, 86, 3, 171]
GRID_NA = [1, 3, 2] * 100
HEADS_NA = [86, 3, 1]
TIMES = (2, 433, T)
SEED = 4321
STATE_KEYS = ("frac_coords", "lattices", "atom_types")
LP = ("log_prob_l", "log_prob_t", "log_prob_x")
HEADS_CAP = dict(x_mid=1e-5, frac_coords=1e-5, lattices=1e-5, atom_types=1e-5, lp_l=1e-4, lp_t=1e-4, lp_x=1e-4)
NETS = {"zero": dict(seed=3, zero_heads=True), "heads": dict(seed=7, zero_heads=False, head_scale=0.1)}


class Device:
    """The library under test: DiffCSPModule.sample / forward_logprb on the GPU.  One network per kind, one module per CSP mode."""

    def __init__(self):
        self.nets = {k: TA._params(2, **kw) for k, kw in NETS.items()}
        self.bias = self.nets["zero"][1]["decoder.type_out.bias"]
        self.cache, self._modules, self._boxes = {}, {}, {}
        self.tables = TA._schedules(self.module("zero"))

    def module(self, net, keep=None):
        if (net, keep) not in self._modules:
            from tests.gpu_util import make_module
            kw = {"coords": dict(cost_coord=0.0), "lattice": dict(cost_lattice=0.0)}.get(keep, {})
            self._modules[net, keep] = make_module(TA.H, 2, TA.F, T, self.nets[net][1], sigmas_norm=R.tables()[1]["sigmas_norm"], **kw)
        return self._modules[net, keep]

    def sample(self, net, na, t_start, t_stop, init=None, z=None, seed=SEED, record=True, streams=1, node_offset=0, graph_offset=0, keep=None):
        """DiffCSPModule.sample.  z: {t: step's z} injected as the [T + 1, ...] noise arrays (None: the device's own draws).  Returns
        (final, traj, rows) on the CPU; rows: the record buffers' log-probability and mid rows at t_start, written or not."""
        from tests.gpu_util import Box
        m = self.module(net, keep)
        B, N = len(na), sum(na)
        noise = None
        if z is not None:
            shapes = dict(corr_x=(N, 3), pred_x=(N, 3), pred_l=(B, 3, 3), pred_t=(N, R.NUM_TYPES))
            noise = {k: torch.zeros(T + 1, *shapes[k], device="cuda") for k in R.NOISE_KEYS}
            for t, zt in z.items():
                for k in R.NOISE_KEYS:
                    noise[k][t] = zt[k].cuda()
        box = self._boxes.setdefault(tuple(na), Box(na))
        sink = [] if record else None
        final, traj = m.sample(box, step_lr=R.STEP_LR, seed=seed, noise=noise, init=init, record=record, t_start=t_start, t_stop=t_stop,
                               node_offset=node_offset, graph_offset=graph_offset, streams=streams, rec_sink=sink)
        torch.cuda.synchronize()
        cpu = lambda d: {k: v.detach().cpu() for k, v in d.items() if torch.is_tensor(v)}
        rows = None
        if record:
            sink.sort(key=lambda e: e[0])
            rows = {k: torch.cat([e[2][k][t_start] for e in sink]).cpu() for k in LP + ("frac_coords_mid",)}
        return cpu(final), {t: cpu(d) for t, d in traj.items()}, rows

    def forward_logprb(self, net, state):
        with torch.no_grad():
            out = self.module(net).forward_logprb(dict(state), step_lr=R.STEP_LR)
        return [v.cpu() for v in out[:3]]


@functools.lru_cache(maxsize=None)
def _dev():
    return Device()


# ---- the harness (dev: Device, or the CPU stand-in of tests/test_sampler_ref64_host.py) ---------------------------------------------------

def _init(state):
    return tuple(state[k] for k in STATE_KEYS)


def _case(dev, net, na, t, seed=17):
    """One state, its noise, scalars and predictions per (network, shape, time): built once per dev, shared, left unchanged."""
    key = (net, tuple(na), t, seed)
    if key not in dev.cache:
        B = len(na)
        s = R.scalars(dev.tables, t, B)
        sz = s if t > 1 else R.scalars(dev.tables, 2, B)         # (t = 1 draws nothing: the injected rows are another step's, to be ignored)
        dev.cache[key] = SimpleNamespace(na=list(na), B=B, N=sum(na), t=t, s=s, s32=R.scalars(dev.tables, t, B, torch.float32),
                                         state=R.build_step_state(na, t, s, seed=seed), z=R.build_noise(na, t, sz, seed=seed + t),
                                         preds=R.zero_head_preds(na, dev.bias) if net == "zero" else None)
    return dev.cache[key]


def _refs(c, z, state=None, **keep):
    state = c.state if state is None else state
    return R.step(c.s, state, c.preds, z, **keep), R.step(c.s32, state, c.preds, z, dtype=torch.float32, **keep)


def _step_checks(what, final, traj, t, r64, r32, slack=None, cap=None):
    """Every quantity of one recorded step t -> t - 1 as _check arguments: the record (x_mid and the log-probabilities at t, where the
    step has them; the state at t - 1) and the returned final state."""
    slack, cap = slack or {}, cap or {}
    rec, nxt = traj[t], traj[t - 1]
    rows = [("record", k, nxt[k]) for k in STATE_KEYS] + [("returned", k, final[k]) for k in STATE_KEYS]
    if "lp_x" in r64:
        rows += [("record", "x_mid", rec["frac_coords_mid"])] + [("record", "lp" + k[-2:], rec[k]) for k in LP]
    return [((d, r64[k], r32[k], f"{what}, {where} {k}"), dict(circle=k in ("x_mid", "frac_coords"), slack=slack.get(k, 0.0), cap=cap.get(k)))
            for where, k, d in rows]


def _assert_state(final, traj, t_stop):
    """The returned state is the recorded one, finite, with the coordinates inside the cell."""
    for k in STATE_KEYS:
        assert torch.equal(final[k], traj[t_stop][k]), k
        assert bool(torch.isfinite(final[k]).all()), k
    assert float(final["frac_coords"].min()) >= 0 and float(final["frac_coords"].max()) < 1


def run_injected(dev, shape, t):
    """Zero heads, injected noise: x_mid, the next state, the three log-probabilities and the returned state against float64; the hair
    elements: the recorded x_mid is the float32 formulas' 1.0f, the predictor's coordinate exactly 0."""
    c = _case(dev, "zero", LOOP_NA if shape == "loop" else GRID_NA, t)
    final, traj, _ = dev.sample("zero", c.na, t, t - 1, init=_init(c.state), z={t: c.z})
    r64, r32 = _refs(c, c.z)
    _all(_step_checks(f"{shape} t={t}", final, traj, t, r64, r32))
    _assert_state(final, traj, t - 1)
    _, _, hc, hp = R.boundary(c.na)
    assert float(traj[t]["frac_coords_mid"].view(-1)[hc]) == float(r32["x_mid"].view(-1)[hc]) == 1.0
    assert float(final["frac_coords"].view(-1)[hp]) == float(r32["frac_coords"].view(-1)[hp]) == 0.0
    assert float(traj[t]["frac_coords_mid"].view(-1)[hp]) == 0.0                      # (x_mid stayed exactly 0 there)


def run_t1(dev):
    """t = 1 on a recording call: no noise is applied (the injected row 1 holds another step's draws: ignored), the state is the
    reference's with z = 0, and the record's log-probability and mid rows of t = 1 still hold the zeros DiffCSPModule._sample_one
    allocates them with (torch.zeros); traj[1] carries no log-probability."""
    c = _case(dev, "zero", LOOP_NA, 1)
    final, traj, rows = dev.sample("zero", c.na, 1, 0, init=_init(c.state), z={1: c.z})
    r64, r32 = _refs(c, None)
    _all(_step_checks("loop t=1", final, traj, 1, r64, r32))
    _assert_state(final, traj, 0)
    assert not any(k in traj[1] for k in LP + ("frac_coords_mid",))
    for k, v in rows.items():
        assert torch.count_nonzero(v) == 0, k


def _philox_slack(c, r64, zg):
    """PHILOX_ATOL x sum |d ref / d z| per quantity: element-wise for the state (std_corr; std_corr + std_pred; sigma), by float64
    autograd for the per-crystal log-probabilities."""
    leaves = list(zg.values())
    sc, sp, sg = (float(c.s[k].max()) for k in ("std_corr", "std_pred", "sigma"))
    out = dict(x_mid=PHILOX_ATOL * sc, frac_coords=PHILOX_ATOL * (sc + sp), lattices=PHILOX_ATOL * sg, atom_types=PHILOX_ATOL * sg)
    out.update({k: _first_order(r64[k], leaves) for k in ("lp_l", "lp_t", "lp_x")})
    return out


def run_device_noise(dev):
    """The device's own draws on a shard that starts at atom NODE_OFF, crystal GRAPH_OFF (inside a Philox quad), t = 433: the reference is
    fed the host contract's draws 3..6 at step 433 with the same offsets."""
    t = 433
    c = _case(dev, "zero", LOOP_NA, t)
    final, traj, _ = dev.sample("zero", c.na, t, t - 1, init=_init(c.state), z=None, seed=SEED, node_offset=NODE_OFF, graph_offset=GRAPH_OFF)
    z = R.philox_noise(SEED, t, c.na, NODE_OFF, GRAPH_OFF)
    zg = {k: v.double().requires_grad_(True) for k, v in z.items()}
    r64 = R.step(c.s, c.state, c.preds, zg)
    r32 = R.step(c.s32, c.state, c.preds, z, dtype=torch.float32)
    _all(_step_checks("device noise on a shard, t=433", final, traj, t, r64, r32, slack=_philox_slack(c, r64, zg)))
    _assert_state(final, traj, t - 1)


def run_init_state(dev):
    """mi_sampler_init_state through sample(t_start = T, t_stop = T) on the same shard against the host contract (draws 0, 1, 2, step
    field T + 1): the project's atol on the draws, the coordinates inside the cell."""
    final, traj, _ = dev.sample("zero", LOOP_NA, T, T, seed=SEED, node_offset=NODE_OFF, graph_offset=GRAPH_OFF)
    ref = dict(zip(STATE_KEYS, R.init_state(SEED, T, LOOP_NA, NODE_OFF, GRAPH_OFF)))
    for k in STATE_KEYS:
        for got in (final[k], traj[T][k]):
            np.testing.assert_allclose(got.numpy(), ref[k].numpy(), rtol=0, atol=PHILOX_ATOL, err_msg=k)
    _assert_state(final, traj, T)


def run_record_vs_not(dev, noise):
    """record=False (lp_corr = NULL, want_lp false) and record=True give the same bits of the final state."""
    t = 433
    c = _case(dev, "zero", LOOP_NA, t)
    kw = dict(z={t: c.z}) if noise == "injected" else dict(z=None, seed=SEED, node_offset=NODE_OFF, graph_offset=GRAPH_OFF)
    a, _, _ = dev.sample("zero", c.na, t, t - 1, init=_init(c.state), record=True, **kw)
    b, _, _ = dev.sample("zero", c.na, t, t - 1, init=_init(c.state), record=False, **kw)
    for k in STATE_KEYS:
        assert torch.equal(a[k], b[k]), k


def run_streams(dev):
    """streams=2 with injected noise (the groups' row slices of the noise arrays) equals streams=1 bit for bit over the two-step chain
    t = 434 -> 432: crystals never interact, and with zero heads the trunk's round-off cannot reach the state."""
    c1, c2 = _case(dev, "zero", LOOP_NA, 434), _case(dev, "zero", LOOP_NA, 433)
    z = {434: c1.z, 433: c2.z}
    fa, ta, _ = dev.sample("zero", c1.na, 434, 432, init=_init(c1.state), z=z, streams=1)
    fb, tb, _ = dev.sample("zero", c1.na, 434, 432, init=_init(c1.state), z=z, streams=2)
    assert sorted(ta) == sorted(tb) == [432, 433, 434]
    for k in STATE_KEYS:
        assert torch.equal(fa[k], fb[k]), k
    for t in ta:
        assert sorted(ta[t]) == sorted(tb[t])
        for k in ta[t]:
            assert torch.equal(ta[t][k], tb[t][k]), (t, k)
    # ... and the first of the two steps is the reference's
    r64, r32 = _refs(c1, c1.z)
    _all([a for a in _step_checks("two streams, t=434", {k: tb[433][k] for k in STATE_KEYS}, tb, 434, r64, r32)])


def run_csp(dev, mode):
    """CSP mode at t = 433, the injected coordinates partly outside the cell (+1, -1): keep_coords -- x_mid and the next coordinates are
    bit-equal to the input mod 1; keep_lattice -- the lattices are bit-equal to the input; everything else matches the reference."""
    t = 433
    c = _case(dev, "zero", LOOP_NA, t)
    x_in = c.state["frac_coords"].clone()
    f = x_in.view(-1)
    f[::5] += 1.0
    f[::7] -= 1.0
    wrapped = x_in % 1.0                                                              # (exact in float32, as pymod1)
    assert float(x_in.min()) < 0 and float(x_in.max()) >= 1 and float(wrapped.min()) >= 0 and float(wrapped.max()) < 1
    state = dict(c.state, frac_coords=wrapped)
    keep = dict(keep_coords=True) if mode == "coords" else dict(keep_lattice=True)
    final, traj, _ = dev.sample("zero", c.na, t, t - 1, init=(x_in, c.state["lattices"], c.state["atom_types"]), z={t: c.z}, keep=mode)
    r64, r32 = _refs(c, c.z, state=state, **keep)
    _all(_step_checks(f"keep {mode}, t=433", final, traj, t, r64, r32))
    _assert_state(final, traj, t - 1)
    assert torch.equal(traj[t]["frac_coords"], wrapped)                               # (the wrap kernels: the state the chain starts from)
    if mode == "coords":
        assert torch.equal(traj[t]["frac_coords_mid"], wrapped) and torch.equal(final["frac_coords"], wrapped)
        assert not torch.equal(final["lattices"], c.state["lattices"])
    else:
        assert torch.equal(final["lattices"], c.state["lattices"]) and not torch.equal(final["frac_coords"], wrapped)


def run_heads(dev, t):
    """head_scale = 0.1 at HEADS_NA: one teacher-forced step against oracle.diffcsp_oracle.sample in float64 (yardstick: the oracle in
    float32, capped at test_teacher_forced_single_steps' bounds), and forward_logprb on the recorded step reproduces the recorded
    log-probabilities at tests/test_gpu_traj_logprob.py's round-trip tolerance (rtol = atol = 1e-4)."""
    c = _case(dev, "heads", HEADS_NA, t, seed=29)
    hp, P = dev.nets["heads"]
    final, traj, _ = dev.sample("heads", c.na, t, t - 1, init=_init(c.state), z={t: c.z})
    refs = []
    for dtype in (torch.float64, torch.float32):
        rec, nxt = R.oracle_step(hp, P, dev.tables, c.state, c.z, t, dtype)
        refs.append(dict(x_mid=rec["frac_coords_mid"], lp_l=rec["log_prob_l"], lp_t=rec["log_prob_t"], lp_x=rec["log_prob_x"], **nxt))
    px = R.network_preds(hp, P, c.s, c.state, c.z, t, torch.float64)
    assert float((c.s["step_pred"][0] * c.s["sqrt_sn"][0] * px[2]).abs().max()) > 0 and float(px[1].abs().max()) > 1e-3
    _all(_step_checks(f"non-zero heads t={t}", final, traj, t, refs[0], refs[1], cap=HEADS_CAP))
    _assert_state(final, traj, t - 1)
    st = dict(atom_types=traj[t]["atom_types"], frac_coords=traj[t]["frac_coords"], frac_coords_mid=traj[t]["frac_coords_mid"],
              lattices=traj[t]["lattices"], next_atom_types=traj[t - 1]["atom_types"], next_frac_coords=traj[t - 1]["frac_coords"],
              next_lattices=traj[t - 1]["lattices"], num_atoms=torch.tensor(c.na), timesteps=torch.full((c.B,), t))
    again = dev.forward_logprb("heads", st)
    for k, v in zip(LP, again):
        np.testing.assert_allclose(v.numpy(), traj[t][k].numpy(), rtol=1e-4, atol=1e-4, err_msg=f"forward_logprb on the recorded step, t={t} {k}")


# ---- the tests ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,t", [("loop", 2), ("loop", 433), ("loop", T), ("grid", 433)])
def test_zero_heads_step_with_injected_noise_vs_float64(shape, t):
    run_injected(_dev(), shape, t)


def test_t1_applies_no_noise_and_records_no_logprob():
    run_t1(_dev())


def test_device_noise_on_a_shard_vs_the_host_philox_contract():
    run_device_noise(_dev())


def test_initial_state_on_a_shard_vs_the_host_philox_contract():
    run_init_state(_dev())


@pytest.mark.parametrize("noise", ["injected", "device"])
def test_recording_changes_no_bit_of_the_state(noise):
    run_record_vs_not(_dev(), noise)


def test_two_streams_with_injected_noise_equal_one_stream():
    run_streams(_dev())


@pytest.mark.parametrize("mode", ["coords", "lattice"])
def test_csp_modes_keep_their_part_bit_for_bit(mode):
    run_csp(_dev(), mode)


@pytest.mark.parametrize("t", TIMES)
def test_nonzero_heads_step_vs_float64_oracle_and_forward_logprb(t):
    run_heads(_dev(), t)
