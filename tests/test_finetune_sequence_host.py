"""CPU-only: the host sequence of finetune.ft_step, path by path, with stand-ins for everything that touches a device.

ft_step runs with a small fake agent / prior on the CPU and with stand-ins on module-level names only (finetune.FusedAdam,
finetune.allreduce_flat_, finetune._fused_micro_step, finetune._stacked_micro_steps, finetune.rank_world, _lib.saturation_events,
streams.concurrent_streams); every stand-in appends to one event list and the tests compare that list with the expected one, entry for
entry: which micro-step is enqueued with which timesteps, shard offsets, noise call ids and auxiliary stream, where the gradient is
all-reduced, where the optimizer steps and zeroes, what closes an epoch.  The gradient's sum is recorded at every micro-step and
all-reduce, so an epoch or a window that started on a gradient that was not zero shows there; HOW an epoch zeroes the (already zero)
gradient at its start -- optimizer.zero_grad or grad.zero_() -- is not an event.

The concurrent-group path needs real streams and is covered by the GPU tests (tests/test_gpu_train.py, tests/test_gpu_optim_clip.py)."""
from types import SimpleNamespace

import pytest
import torch

from matinvent_amd import _lib, finetune, streams
from matinvent_amd.data import CrystalData

NA = [4, 2, 6, 3]
P = 5                     # parameters of the fake network
CFG = dict(lr=1e-4, accum_steps=3, epochs=2, timesteps=7, sigma=0.025)
STEP = [("step",), ("zero_grad",)]
KEYS = ["loss", "loss_diff", "loss_kl"]
GRAD_KEYS = ["grad_norm", "grad_norm_max", "clipped_steps", "skipped_steps"]


class FakeModule:
    """The module surface ft_step's autograd loop drives; the fused paths only read `decoder.theta`, `device` and call train()."""

    def __init__(self, ev, name, trainable=True):
        self.ev, self.name = ev, name
        self.device = torch.device("cpu")
        self.decoder = SimpleNamespace(theta=torch.nn.Parameter(torch.zeros(P), requires_grad=trainable))
        self.training = False

    def train(self):
        self.training = True

    def add_noise(self, batch, t, noise=None):
        self._noise_calls = getattr(self, "_noise_calls", 0) + 1
        self.ev.append(("add_noise", t, self.shard_offsets, self._noise_calls, noise, len(batch.reward)))
        return SimpleNamespace(batch=batch)

    def calc_sample_loss(self, noised):
        self.ev.append((self.name + ".calc_sample_loss", self.shard_offsets))
        n = len(noised.batch.reward)
        return self.decoder.theta.sum() * torch.ones(n) + 1.0, torch.ones(n)

    def calc_kl_reg(self, agent_pred, prior_pred, batch):
        return agent_pred * 0.0 + 2.0

    def predict(self, noised):
        self.ev.append((self.name + ".predict",))
        raise AssertionError("the module-surface loop on this device evaluates through calc_sample_loss")


class FakeCollatingModule(FakeModule):
    def collate(self, data, rewards):
        batch = SimpleNamespace(reward=torch.as_tensor(rewards, dtype=torch.float32), n=len(data))
        batch.to = lambda device: batch
        return batch


class Harness:
    def __init__(self, monkeypatch, rank_world=(0, 1), collating=False):
        self.ev, self.adams, self.logs = [], [], []
        ev, adams = self.ev, self.adams
        self.agent = (FakeCollatingModule if collating else FakeModule)(ev, "agent")
        self.prior = (FakeCollatingModule if collating else FakeModule)(ev, "prior", trainable=False)
        theta = self.agent.decoder.theta
        theta.register_hook(lambda g: ev.append(("backward",)))

        class Adam:
            def __init__(self, params, lr, **kw):
                assert len(params) == 1 and params[0] is theta
                adams.append((lr, kw))
                self.guarded = kw.get("max_grad_norm") is not None or bool(kw.get("skip_nonfinite"))
                self.stepped = False

            def step(self):
                ev.append(("step",))
                self.stepped = True

            def zero_grad(self, set_to_none=True):
                assert set_to_none is False
                if self.stepped:      # (the zeroing that belongs to an optimizer step; an epoch's start on a zero gradient is no event)
                    ev.append(("zero_grad",))
                self.stepped = False
                if theta.grad is not None:
                    theta.grad.zero_()

            def grad_stats(self, reset=False):
                assert reset is True
                ev.append(("grad_stats",))
                return torch.zeros(8, dtype=torch.float64)

        def allreduce(buf):
            if theta.grad is not None and buf.data_ptr() == theta.grad.data_ptr():
                ev.append(("allreduce", "grad", float(buf.sum())))
            else:
                ev.append(("allreduce", "epoch", buf.numel()))
            return buf

        def micro(agent, prior, batch, time_idx, noise, sigma, n_global, accum_steps, grad, stats, call_id=None, aux_stream=None):
            assert agent.training and call_id is None and grad is theta.grad
            agent._noise_calls = getattr(agent, "_noise_calls", 0) + 1
            ev.append(("micro", time_idx, 1, agent.shard_offsets, prior.shard_offsets, agent._noise_calls, aux_stream, noise,
                       (sigma, n_global, accum_steps), batch.num_graphs, float(grad.sum())))
            grad += 1.0
            stats += torch.tensor([1.0, 2.0, 3.0])

        def stacked(agent, prior, batch, time_idxs, noises, sigma, n_global, accum_steps, grad, stats, aux_stream=None):
            assert agent.training and grad is theta.grad
            k = len(time_idxs)
            agent._noise_calls = getattr(agent, "_noise_calls", 0) + k
            ev.append(("stacked", list(time_idxs), k, agent.shard_offsets, prior.shard_offsets, agent._noise_calls, aux_stream, noises,
                       (sigma, n_global, accum_steps), batch.num_graphs, float(grad.sum())))
            grad += float(k)
            stats += k * torch.tensor([1.0, 2.0, 3.0])

        def saturation_events(reset=False):
            assert reset is True
            ev.append(("saturation",))
            return 0

        monkeypatch.setattr(finetune, "FusedAdam", Adam)
        monkeypatch.setattr(finetune, "allreduce_flat_", allreduce)
        monkeypatch.setattr(finetune, "_fused_micro_step", micro)
        monkeypatch.setattr(finetune, "_stacked_micro_steps", stacked)
        monkeypatch.setattr(finetune, "rank_world", lambda: rank_world)
        monkeypatch.setattr(_lib, "saturation_events", saturation_events)
        monkeypatch.setattr(streams, "concurrent_streams", lambda n, device=None: [f"stream{i}" for i in range(n)])

    def run(self, data, cfg, **kw):
        rewards = [0.5] * len(data)
        return finetune.ft_step(self.agent, self.prior, data, rewards, cfg, log=self.logs.append, **kw)


def _crystals(na=NA):
    g = torch.Generator().manual_seed(0)
    return [CrystalData(torch.rand(n, 3, generator=g), torch.randint(1, 95, (n,), generator=g), 5 + torch.rand(1, 3, generator=g),
                        80 + 20 * torch.rand(1, 3, generator=g)) for n in na]


def _fused_epoch(chunks, first_call, noise_of=None, accum=3, n_global=len(NA)):
    """The expected events of one single-group epoch whose micro-steps take `chunks` timesteps each."""
    out, t0, call, g = [], 0, first_call, 0.0
    for k in chunks:
        tidx = list(range(t0, t0 + k))
        call += k
        args = ((0, 0), (0, 0), call, "stream1")
        tail = ((0.025, n_global, accum), n_global, g)
        if k == 1:
            out.append(("micro", t0, 1) + args + (None if noise_of is None else noise_of(t0),) + tail)
        else:
            out.append(("stacked", tidx, k) + args + (None if noise_of is None else [noise_of(i) for i in tidx],) + tail)
        t0 += k
        g += P * k
        if t0 % accum == 0 or t0 == sum(chunks):
            out += [("allreduce", "grad", g)] + STEP
            g = 0.0
    return out + [("saturation",), ("allreduce", "epoch", 4)]


def _check_fused(h, stats, timesteps):
    assert [list(d) for d in stats] == [KEYS, KEYS]
    for d in stats:   # the stand-in micro-steps add (1, 2, 3) per timestep to the accumulators
        assert d == dict(loss=1.0, loss_diff=2.0 / len(NA), loss_kl=3.0 / len(NA))
    assert h.adams == [(1e-4, dict(max_grad_norm=None, skip_nonfinite=False))]
    assert len(h.logs) == 2 and h.logs[0].startswith("Epoch 0: loss: 1.0000") and h.logs[1].startswith("Epoch 1: ")
    assert h.agent._noise_calls == 2 * timesteps
    assert h.agent.decoder.theta.grad is not None and float(h.agent.decoder.theta.grad.abs().sum()) == 0.0


@pytest.mark.parametrize("stack,chunks", [(None, [3, 3, 1]), (2, [2, 1, 2, 1, 1])], ids=["a-stack-auto", "b-stack-2"])
def test_single_group_fused_with_a_tail_window(monkeypatch, stack, chunks):
    """(a), (b): 7 timesteps in windows of 3: every chunk inside one window, k == 1 through the single entry, three optimizer steps per
    epoch (the last one on the partial window), k consecutive noise call ids per chunk, the prior's stream = concurrent_streams(2)[1]."""
    h = Harness(monkeypatch)
    stats = h.run(_crystals(), CFG, stack=stack)
    assert h.ev == _fused_epoch(chunks, 0) + _fused_epoch(chunks, 7)
    assert sum(e == ("step",) for e in h.ev) == 6
    _check_fused(h, stats, 7)


def test_single_group_fused_without_a_tail_window(monkeypatch):
    """(c): 6 timesteps in windows of 3: no step behind the last full window; injected noise reaches each micro-step as noise_fn(epoch, t)
    of its own timesteps."""
    h = Harness(monkeypatch)
    stats = h.run(_crystals(), dict(CFG, timesteps=6), noise_fn=lambda e, t: ("noise", e, t))
    want = [_fused_epoch([3, 3], 6 * e, noise_of=lambda t, e=e: ("noise", e, t)) for e in range(2)]
    assert h.ev == want[0] + want[1]
    assert sum(e == ("step",) for e in h.ev) == 4
    _check_fused(h, stats, 6)


def test_empty_shard_keeps_the_collectives_and_the_optimizer_options(monkeypatch):
    """(d): rank 1 of 2 with one crystal: nothing to differentiate, ceil(7 / 3) all-reduce / step pairs per epoch on a zero gradient,
    the noise call counter advanced by 7 per epoch, the clipping options on the optimizer, epoch dicts of zeros, no log line."""
    h = Harness(monkeypatch, rank_world=(1, 2))
    stats = h.run(_crystals([4]), dict(CFG, max_grad_norm=2.0, skip_nonfinite_steps=True))
    epoch = ([("allreduce", "grad", 0.0)] + STEP) * 3 + [("saturation",), ("grad_stats",), ("allreduce", "epoch", 12)]
    assert h.ev == epoch + epoch
    assert h.adams == [(1e-4, dict(max_grad_norm=2.0, skip_nonfinite=True))]
    assert h.agent._noise_calls == 14
    assert [list(d) for d in stats] == [KEYS + GRAD_KEYS] * 2
    assert all(v == 0 for d in stats for v in d.values())
    assert h.logs == []
    assert h.agent.decoder.theta.grad is not None and h.agent.decoder.theta.grad.shape == (P,)


def _surface_epoch(chunks, first_call, noise_of=None, timesteps=7, accum=3):
    """The expected events of one module-surface epoch over `chunks` = [(crystals, shard offsets)]."""
    out = []
    for t in range(timesteps):
        for n, offs in chunks:   # every chunk of a timestep draws with the same call id
            out += [("add_noise", t, offs, first_call + t + 1, None if noise_of is None else noise_of(t), n),
                    ("agent.calc_sample_loss", offs), ("prior.calc_sample_loss", offs), ("backward",)]
        if (t + 1) % accum == 0 or t + 1 == timesteps:
            out += [("allreduce", "grad")] + STEP
    return out + [("saturation",), ("allreduce", "epoch", 4)]


def _surface_events(h):
    return [e[:2] if e[:2] == ("allreduce", "grad") else e for e in h.ev]


def test_module_surface_in_chunks(monkeypatch):
    """(e): an agent with `collate`, FT_CHUNK_ATOMS = 9 -> crystals [4, 2] and [6, 3]: per timestep one add_noise / forward pair / backward
    per chunk with the chunk's shard offsets, the noise call counter restored so that both chunks use one id, steps at the window ends."""
    import matinvent_amd.mattergen as MG
    monkeypatch.setattr(MG, "FT_CHUNK_ATOMS", 9)
    h = Harness(monkeypatch, collating=True)
    data = [SimpleNamespace(num_atoms=n) for n in NA]
    stats = h.run(data, CFG)
    chunks = [(2, (0, 0)), (2, (6, 2))]
    assert _surface_events(h) == _surface_epoch(chunks, 0) + _surface_epoch(chunks, 7)
    assert sum(e == ("backward",) for e in h.ev) == 2 * 7 * 2 and sum(e == ("step",) for e in h.ev) == 6
    assert h.agent._noise_calls == 14
    assert [list(d) for d in stats] == [KEYS, KEYS] and len(h.logs) == 2
    # loss = sum_b (0.5 * 1 + 0.025 * 2 * 0.6) / (4 * 3) per timestep, logged x accum_steps, / timesteps
    assert stats[0]["loss"] == pytest.approx(4 * (0.5 + 0.025 * 2.0 * 0.6) / 4, rel=1e-6)
    assert stats[0]["loss_diff"] == pytest.approx(0.5, rel=1e-6) and stats[0]["loss_kl"] == pytest.approx(1.2, rel=1e-6)
    assert h.adams == [(1e-4, dict(max_grad_norm=None, skip_nonfinite=False))]


def test_module_surface_with_injected_noise_is_one_chunk(monkeypatch):
    """(f): injected noise spans the shard, so the same set stays one chunk whatever FT_CHUNK_ATOMS says."""
    import matinvent_amd.mattergen as MG
    monkeypatch.setattr(MG, "FT_CHUNK_ATOMS", 9)
    h = Harness(monkeypatch, collating=True)
    data = [SimpleNamespace(num_atoms=n) for n in NA]
    h.run(data, CFG, noise_fn=lambda e, t: ("noise", e, t))
    want = [_surface_epoch([(4, (0, 0))], 7 * e, noise_of=lambda t, e=e: ("noise", e, t)) for e in range(2)]
    assert _surface_events(h) == want[0] + want[1]
    assert sum(e == ("backward",) for e in h.ev) == 14


def test_diffcsp_autograd_surface_evaluates_the_prior_through_calc_sample_loss(monkeypatch):
    """(g): fused=False on a module without `collate`: one batch with the shard's offsets, the prior through calc_sample_loss, never
    through predict (which the fake has, as DiffCSPModule has)."""
    h = Harness(monkeypatch)
    stats = h.run(_crystals(), CFG, fused=False)
    assert _surface_events(h) == _surface_epoch([(4, (0, 0))], 0) + _surface_epoch([(4, (0, 0))], 7)
    assert not any(e[0].endswith(".predict") for e in h.ev)
    assert sum(e == ("prior.calc_sample_loss", (0, 0)) for e in h.ev) == 14
    assert h.agent._noise_calls == 14 and [list(d) for d in stats] == [KEYS, KEYS]


@pytest.mark.parametrize("missing", ["lr", "accum_steps", "epochs", "timesteps", "sigma"])
def test_a_config_without_a_required_key_raises_before_any_work(monkeypatch, missing):
    """(h): nothing is constructed, enqueued or reduced for a config that lacks one of the five required entries."""
    h = Harness(monkeypatch)
    cfg = {k: v for k, v in CFG.items() if k != missing}
    with pytest.raises((KeyError, AttributeError, ValueError)):
        h.run(_crystals(), cfg)
    assert h.ev == [] and h.adams == [] and h.logs == []
    assert h.agent.decoder.theta.grad is None and not hasattr(h.agent, "_noise_calls")
