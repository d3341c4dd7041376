"""GPU checks of the resampling jumps (matinvent_amd/csrc/resample.hip, include/matinvent_hip_resample.h) on the 64-wide,
2-layer network of tests/test_gpu_respaced_chain.py with T = 20:

1. mi_resample_jump against the float64 restatement tests/resample_ref64.py at the sizes the kernel loops over;
2. a resampled chain IS unconditioned single steps, impositions and jumps in schedule order under the visit seeds, bit for bit, on the
   full grid and on a view;
3. r = 1, and a handle that carried resampling before, change nothing;
4. after a full chain the known part is exact, and the free part is not the r = 1 chain's;
5. split batches (bit for bit);
6. what mi_sampler_run refuses, with nothing enqueued;
7. DiffCSPSampler.generate with resample_times / jump_length and one drop-in MatInvent loop with the two keys.

Tolerance of (1): tests/test_gpu_condition.py's `_close` -- the yardstick of a quantity is the deviation of the float32 formulas run on the
CPU (resample_ref64.jump in float32: the same separately rounded ops, same draws, the float32 table the device gets) from float64,
relative to max|ref64|; the device gets 4 times that, at least 4 * 2^-24, plus 5e-6 x |d out / d z| = 5e-6 c1 (types, lattice) or 5e-6 s
(coordinates) for the Box-Muller libm round-off of the device's own draws.  Coordinates are compared on the circle, scale 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import tests.test_gpu_condition as GC
import tests.test_gpu_respaced_chain as RC
from matinvent_amd import _lib, conditioning, resampling as RS
from matinvent_amd.conditioning import Condition
from matinvent_amd.cspnet import _ptr, _stream
from matinvent_amd.structure import reduced_formula
from tests import resample_ref64 as R
from tests.gpu_util import Box

pytestmark = pytest.mark.gpu

T = 20
STEP_LR = RC.STEP_LR
NA = RC.NA                                   # [1, 3, 7]
LOOP_NA, GRID_NA = GC.LOOP_NA, GC.GRID_NA    # the second trip of the four-wave type loop and of the 256-thread coordinate loop; 300 blocks
NODE_OFF, GRAPH_OFF = GC.NODE_OFF, GC.GRAPH_OFF
SEED = 4321
STATE = ("atom_types", "frac_coords", "lattices")


@pytest.fixture(scope="module")
def base():
    return RC._base()[0]


def _state(na, seed):
    """A random state whose coordinates lie in [0, 1), the first exactly 0 and the last nextafter(1, 0)."""
    a, x, l = GC._state(na, seed)
    x.view(-1)[0], x.view(-1)[-1] = 0.0, float(np.nextafter(np.float32(1), np.float32(0)))
    return a, x, l


# ---- 1. the kernel against float64 --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("j", [1, 3])
@pytest.mark.parametrize("shape", ["loop", "grid"])
def test_resample_jump_against_float64(base, shape, j):
    na = {"loop": LOOP_NA, "grid": GRID_NA}[shape]
    cb = base.make_batch(na, NODE_OFF, GRAPH_OFF)
    RS.attach(base, cb, 3, j)
    t64, t32 = R.jump_table(GC._tables(base), j), RS.jump_table(base, j)
    assert torch.equal(t32, t64.float())
    for level in (0, 1, 7, T - j):
        before = _state(na, seed=30 + level)
        dev = tuple(v.cuda().contiguous() for v in before)
        RS.jump(cb, level, SEED, *dev)
        torch.cuda.synchronize()
        a, x, l = (v.cpu() for v in dev)
        z = R.draws(SEED, level + j, na, NODE_OFF, GRAPH_OFF)
        r64, r32 = R.jump(before, t64, level, z), R.jump(before, t32, level, z, dtype=torch.float32)
        c1, s = float(t64[level, 1]), float(t64[level, 2])
        what = f"{shape} j = {j} level {level}"
        GC._close(a, r64[0], r32[0], GC.PHILOX_ATOL * c1, what + " atom_types")
        GC._close(x, r64[1], r32[1], GC.PHILOX_ATOL * s, what + " frac_coords", circle=True)
        GC._close(l, r64[2], r32[2], GC.PHILOX_ATOL * c1, what + " lattices")
        # a jump knows no mask: every element moved; the coordinates stay in the cell
        assert not (a == before[0]).any() and not (x == before[1]).any() and not (l == before[2]).any(), what
        assert float(x.min()) >= 0.0 and float(x.max()) < 1.0, what
    with pytest.raises(_lib.MIError, match="outside") as e:   # a level whose target lies outside the table
        RS.jump(cb, T - j + 1, SEED, *dev)
    assert e.value.code == _lib.MI_EINVAL
    with pytest.raises(_lib.MIError, match="outside") as e:
        RS.jump(cb, -1, SEED, *dev)
    assert e.value.code == _lib.MI_EINVAL
    RS.clear(cb)
    with pytest.raises(_lib.MIError, match="no resampling") as e:   # no resampling on the handle
        RS.jump(cb, 1, SEED, *dev)
    assert e.value.code == _lib.MI_EINVAL
    torch.cuda.synchronize()
    assert all(torch.equal(p.cpu(), q) for p, q in zip(dev, (a, x, l)))   # the refused calls wrote nothing


# ---- 2. the chain is single steps, impositions and jumps ----------------------------------------------------------------------------

@pytest.mark.parametrize("S,t_start,rj", [(None, 7, (3, 3)), (5, 5, (2, 2))])
def test_resampled_chain_is_steps_impositions_and_jumps(base, S, t_start, rj):
    v = base if S is None else base.respaced(S)
    Tv = v.beta_scheduler.timesteps
    r, j = rj
    c = GC._cond(NA, seed=32)
    assert c.known_types.any() and c.known_coords.any() and c.known_lattice.any() and not c.known_types.all() and not c.known_lattice.all()
    seed = 41
    final, _ = v.sample(c, step_lr=STEP_LR, seed=seed, streams=1, t_start=t_start, condition=c, resample=rj)
    lib = _lib.load()
    cb = v.make_batch(NA)
    c.attach(v, cb)
    RS.attach(v, cb, r, j)
    N, B = sum(NA), len(NA)
    x, l, a = torch.empty(N, 3, device="cuda"), torch.empty(B, 3, 3, device="cuda"), torch.empty(N, 100, device="cuda")
    _lib.check(lib.mi_sampler_init_state(cb._h, seed, Tv, _ptr(a), _ptr(x), _ptr(l), _stream()))
    conditioning.apply(cb, t_start, seed, a, x, l)
    cur = dict(atom_types=a, frac_coords=x, lattices=l)
    box = Box(NA)
    moves = RS.walk(t_start, r, j, seed)
    assert sum(k == "jump" for k, _, _ in moves) > 0 and len({sv for _, _, sv in moves}) == r
    for kind, t, sv in moves:
        if kind == "step":
            f, _ = v.sample(box, step_lr=STEP_LR, seed=sv, streams=1, init=(cur["frac_coords"], cur["lattices"], cur["atom_types"]), t_start=t,
                            t_stop=t - 1)
            conditioning.apply(cb, t - 1, sv, f["atom_types"], f["frac_coords"], f["lattices"])
            cur = {k: f[k] for k in STATE}
        else:
            RS.jump(cb, t, sv, cur["atom_types"], cur["frac_coords"], cur["lattices"])
    for k in STATE:
        assert torch.equal(final[k], cur[k]), k
    Condition.clear(cb)
    RS.clear(cb)


# ---- 3. r = 1 changes nothing -------------------------------------------------------------------------------------------------------

def test_r_one_and_a_cleared_handle_change_nothing(base):
    c = GC._cond(NA, seed=52)
    kw = dict(step_lr=STEP_LR, seed=53, streams=1, t_start=6, condition=c)
    plain = base.sample(c, **kw)[0]
    one = base.sample(c, resample=(1, 3), **kw)[0]
    for k in STATE:
        assert torch.equal(plain[k], one[k]), k
    jumped = base.sample(c, resample=(2, 3), **kw)[0]            # the same cached handle, resampled ...
    assert not c.known_coords.all() and not torch.equal(jumped["frac_coords"], plain["frac_coords"])
    again = base.sample(c, **kw)[0]                               # ... and not any more
    for k in STATE:
        assert torch.equal(plain[k], again[k]), k


# ---- 4. exact at the end ------------------------------------------------------------------------------------------------------------

def test_known_part_is_exact_after_a_full_resampled_chain(base):
    c = GC._cond(NA, seed=51)
    final, _ = base.sample(c, step_lr=STEP_LR, seed=61, streams=1, condition=c, resample=(3, 4))
    plain, _ = base.sample(c, step_lr=STEP_LR, seed=61, streams=1, condition=c)
    a, x, l = (final[k].cpu() for k in STATE)
    kt, kx, kl = c.known_types, c.known_coords, c.known_lattice
    assert kt.any() and kx.any() and kl.any() and (~kt).any() and (~kx).any() and (~kl).any()
    assert torch.equal(a[kt], torch.nn.functional.one_hot(c.atom_types[kt] - 1, 100).float())
    assert torch.equal(x[kx], c.frac_coords[kx]) and torch.equal(l[kl], c.lattices[kl])
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(x).all()) and bool(torch.isfinite(l).all())
    pa, px, pl = (plain[k].cpu() for k in STATE)
    assert not torch.equal(a[~kt], pa[~kt]) and not torch.equal(x[~kx], px[~kx]) and not torch.equal(l[~kl], pl[~kl])
    assert torch.equal(a[kt], pa[kt]) and torch.equal(x[kx], px[kx]) and torch.equal(l[kl], pl[kl])


# ---- 5. splits ----------------------------------------------------------------------------------------------------------------------

def test_split_batches_draw_the_same_numbers(base):
    na = NA + NA[::-1]
    c = GC._cond(na, seed=81)
    kw = dict(step_lr=STEP_LR, seed=82, t_start=7, resample=(2, 3))
    two = base.sample(Box(na), streams=2, condition=c, **kw)[0]
    h, n0 = len(na) // 2, sum(na[:len(na) // 2])
    seq = [base.sample(Box(na[:h]), streams=1, condition=c.slice(0, h), **kw)[0],
           base.sample(Box(na[h:]), streams=1, node_offset=n0, graph_offset=h, condition=c.slice(h, len(na)), **kw)[0]]
    for k in STATE:
        assert torch.equal(torch.cat([s_[k] for s_ in seq]), two[k]), k
    other = base.sample(Box(na[h:]), streams=1, condition=c.slice(h, len(na)), **kw)[0]      # without its offsets: other numbers
    assert not torch.equal(other["lattices"], seq[1]["lattices"])


# ---- 6. refusals on the device ------------------------------------------------------------------------------------------------------

def _run(v, cb, state, t_start, t_stop=0, noise=None, rec=None, seed=7):
    """mi_sampler_run itself on the caller's arrays (atom_types, frac, lattices): its return code."""
    lib = _lib.load()
    Tv = v.beta_scheduler.timesteps
    v.decoder.sync()
    coef = v._coefficients(STEP_LR)
    a, x, l = state
    return lib.mi_sampler_run(v.decoder._h, cb._h, coef.numpy().ctypes.data_as(C.POINTER(C.c_float)), Tv, t_start, t_stop,
                              _ptr(v.time_embedding.freqs), seed, C.byref(noise) if noise is not None else None,
                              C.byref(rec) if rec is not None else None, _ptr(a), _ptr(x), _ptr(l), _stream())


def test_sampler_run_refusals_enqueue_nothing(base):
    lib = _lib.load()
    c = GC._cond(NA, seed=91)
    N, B = sum(NA), len(NA)
    host = _state(NA, 92)
    state = tuple(v.cuda().contiguous() for v in host)
    cb = base.make_batch(NA)
    z = lambda *s: torch.zeros(*s, device="cuda")
    keep = [z(T + 1, N, 100), z(T + 1, N, 3), z(T + 1, B, 3, 3), z(T + 1, N, 3), z(T + 1, B), z(T + 1, B), z(T + 1, B)]
    rec = _lib.SamplerRecord(*(t.data_ptr() for t in keep))
    nz = [z(T + 1, N, 3), z(T + 1, B, 3, 3), z(T + 1, N, 100), z(T + 1, N, 3)]
    noise = _lib.SamplerNoise(*(t.data_ptr() for t in nz))

    def refused(match, **kw):
        torch.cuda.synchronize()
        rc = _run(base, cb, state, **{"t_start": 7, **kw})
        msg = lib.mi_last_error().decode()
        torch.cuda.synchronize()
        assert rc == _lib.MI_EINVAL and match in msg, (rc, msg)
        assert all(torch.equal(p.cpu(), q) for p, q in zip(state, host)), match     # nothing was enqueued: the state is bit-unchanged
        assert all(not bool(t.any()) for t in keep)

    RS.attach(base, cb, 2, 3)
    refused("no condition")
    c.attach(base, cb)
    refused("recorded", rec=rec)
    refused("teacher-forced", noise=noise)
    refused("t_stop", t_stop=1)
    refused("no jump-off level", t_start=3)
    c.attach_likelihood(base, cb)
    refused("likelihood mask")
    Condition.clear_likelihood(cb)
    RS.attach(base, cb, 2, 3, table=RS.jump_table(base, 3)[:T])
    refused("jump table")
    # a refused attach leaves the handle as it was: still the short table
    tab = RS.jump_table(base, 3)
    for bad in (dict(r=0, j=3), dict(r=2, j=0), dict(r=2, j=T + 1)):
        with pytest.raises(_lib.MIError) as e:
            RS.attach(base, cb, bad["r"], bad["j"], table=tab)
        assert e.value.code == _lib.MI_EINVAL
    refused("jump table")
    # r = 1 on the handle is the plain chain: none of the above applies, and with (2, 3) and everything in order the chain runs
    RS.attach(base, cb, 1, 3)
    assert _run(base, cb, tuple(v.clone() for v in state), t_start=2, t_stop=1, rec=rec) == 0
    RS.attach(base, cb, 2, 3)
    moved = tuple(v.clone() for v in state)
    assert _run(base, cb, moved, t_start=7) == 0
    torch.cuda.synchronize()
    assert not torch.equal(moved[2], state[2]) and bool(torch.isfinite(moved[0]).all())
    Condition.clear(cb)
    RS.clear(cb)


# ---- 7. surface ---------------------------------------------------------------------------------------------------------------------

def test_generate_with_resample_times_and_jump_length(base, monkeypatch):
    from matinvent_amd.diffcsp import DiffCSPModule
    from matinvent_amd.sampling import DiffCSPSampler
    seen = []
    real = DiffCSPModule.sample

    def spy(self, *a, **kw):
        seen.append(kw.get("resample"))
        return real(self, *a, **kw)

    monkeypatch.setattr(DiffCSPModule, "sample", spy)
    data, strucs = DiffCSPSampler(seed=5).generate(base, target_compositions_dict=GC.TARGETS, batch_size=4, num_batches=1, resample_times=2,
                                                   jump_length=5)
    assert len(data) == len(strucs) == 4 and seen == [(2, 5)]
    assert [reduced_formula(d.atom_types.tolist()) for d in data] == GC.FORMULAS * 2
    plain, _ = DiffCSPSampler(seed=5).generate(base, target_compositions_dict=GC.TARGETS, batch_size=4, num_batches=1)
    assert seen == [(2, 5), None]
    assert not torch.equal(plain[0].frac_coords, data[0].frac_coords)


def test_dropin_mat_invent_pipeline_with_resampling(tmp_path, monkeypatch):
    """pipeline=mat_invent through dropin/main.py with sample_cfg.resample_times / jump_length beside target_compositions_dict (and
    sample_steps = 5, so the levels are the view's step indices): the chains are resampled and the loop runs to its log line."""
    from matinvent_amd.diffcsp import DiffCSPModule
    seen = []
    real = DiffCSPModule.sample

    def spy(self, *a, **kw):
        seen.append((self.beta_scheduler.timesteps, kw.get("resample")))
        return real(self, *a, **kw)

    monkeypatch.setattr(DiffCSPModule, "sample", spy)
    rl = RC._run_dropin(tmp_path, ["expname=resample", "model.finetune_cfg.timesteps=6", "pipeline.finetune_cfg.accum_steps=3",
                                   "pipeline.finetune_cfg.epochs=1", "+sample_cfg.target_compositions_dict=[{Li: 2, O: 1}, {Na: 1, Cl: 1}]",
                                   "+sample_cfg.resample_times=2", "+sample_cfg.jump_length=2"])
    assert rl.sample_cfg.resample_times == 2 and rl.sample_cfg.jump_length == 2
    assert seen and all(s == (5, (2, 2)) for s in seen)
    rows = (tmp_path / "exp_res" / "resample" / "metrics.csv").read_text().strip().splitlines()
    assert len(rows) == 2 and "reward mean" in rows[0]
