"""CPU checks of the resampling layer that needs no GPU (matinvent_amd.resampling, include/matinvent_hip_resample.h): the
schedule against RePaint's published algorithm and the library's definition, the per-visit seeds against the oracle's Philox words, that no
(seed, level, draw id) occurs twice in a chain, the float64 identities that make a jump consistent with the forward process, the header's
symbols and the host-side refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from matinvent_amd import _lib, resampling as RS
from matinvent_amd.conditioning import Condition
from oracle import diffcsp_oracle as O
from tests import resample_ref64 as R
from tests.header_util import declared_symbols

CASES = [(20, 3, 4), (20, 1, 5), (6, 2, 1), (20, 10, 10), (250, 10, 10), (7, 3, 3)]
KNOWN = {(20, 3, 4): (52, 8), (250, 10, 10): (2410, 216), (7, 3, 3): (19, 4)}    # (reverse steps, jumps)


def _module(T=20):
    from matinvent_amd.diffcsp import DiffCSPModule
    return DiffCSPModule(decoder=dict(hidden_dim=64, num_layers=2, num_freqs=8, ln=True, edge_style="fc"),
                         beta_scheduler=dict(timesteps=T, scheduler_mode="cosine"),
                         sigma_scheduler=dict(timesteps=T, sigma_begin=0.005, sigma_end=0.5, sigmas_norm=torch.linspace(0.7, 1.3, T + 1)),
                         device="cpu")


def _tables(m):
    return dict(alphas_cumprod=m.beta_scheduler.alphas_cumprod.cpu(), sigmas=m.sigma_scheduler.sigmas.cpu())


# ---- the schedule -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES)
def test_schedule_is_repaints_and_the_librarys(case):
    t_start, r, j = case
    levels = RS.schedule(t_start, r, j)
    assert levels == RS.library_schedule(t_start, r, j)
    assert R.expand(levels, j) == R.repaint_levels(t_start, j, r)
    assert levels[0] == t_start and levels[-1] == 0 and min(levels) == 0 and max(levels) == t_start
    moves = list(zip(levels[:-1], levels[1:]))
    steps, jumps = [a for a, b in moves if b == a - 1], [a for a, b in moves if b == a + j]
    assert len(steps) + len(jumps) == len(moves)
    if case in KNOWN:
        assert (len(steps), len(jumps)) == KNOWN[case]
    if r == 1:
        assert levels == list(range(t_start, -1, -1))
    # no transition runs more than r times, the last one once; a jump-off level is left r - 1 times, level 0 never
    assert max(steps.count(t) for t in set(steps)) <= r and steps.count(1) == 1 and 0 not in jumps
    offs = [L for L in range(1, t_start + 1, j) if L + j <= t_start]
    assert sorted(set(jumps)) == (offs if r > 1 else []) and all(jumps.count(L) == r - 1 for L in offs)
    # a capped read fills the head of the list and still returns the whole length
    buf = np.full(5, -7, dtype=np.int32)
    n = _lib.load().mi_resample_schedule(t_start, r, j, buf.ctypes.data_as(C.POINTER(C.c_int)), 3)
    assert n == len(levels) and buf.tolist() == levels[:3] + [-7, -7]


def test_the_known_visit_list():
    assert RS.schedule(7, 3, 3) == [7, 6, 5, 4, 7, 6, 5, 4, 7, 6, 5, 4, 3, 2, 1, 4, 3, 2, 1, 4, 3, 2, 1, 0]


@pytest.mark.parametrize("case", CASES)
def test_no_seed_level_draw_triple_occurs_twice(case):
    """Every draw of a chain is keyed by (seed_v, step field, draw id): the transition t -> t - 1 draws ids 3..6 at step t, the imposition
    after it ids 21..23 at step t - 1, a jump to b ids 24..26 at step b; the initial draw ids 0..2 at T + 1 and the first imposition at
    t_start under the chain's seed.  (visit, level, kind) never repeats, and distinct visits have distinct seeds."""
    t_start, r, j = case
    seed = 0x1234567812345678
    seeds = [RS.visit_seed(seed, v) for v in range(r + 1)]
    assert len(set(seeds)) == r + 1 and seeds[0] == seed
    visit = {s: v for v, s in enumerate(seeds)}
    seen = [(seed, t_start + 1, d) for d in (0, 1, 2)] + [(seed, t_start, d) for d in (21, 22, 23)]
    kinds = []
    for kind, level, sv in RS.walk(t_start, r, j, seed):
        kinds.append((visit[sv], level, kind))
        if kind == "step":
            seen += [(sv, level, d) for d in (3, 4, 5, 6)] + [(sv, level - 1, d) for d in (21, 22, 23)]
        else:
            assert visit[sv] >= 1
            seen += [(sv, level + j, d) for d in (R.DRAW_JUMP_L, R.DRAW_JUMP_X, R.DRAW_JUMP_T)]
    assert len(set(seen)) == len(seen) and len(set(kinds)) == len(kinds)
    if r == 1:
        assert {s for s, _, _ in seen} == {seed}
    first = [m for m in RS.walk(t_start, r, j, seed) if m[0] == "step"]
    assert first[0] == ("step", t_start, seed)


# ---- the visit seed -----------------------------------------------------------------------------------------------------------------

def test_visit_seed_is_the_oracles_philox_words():
    lib = _lib.load()
    for seed in (1234, 0xFEDCBA9876543210):
        for v in (0, 1, 2, 2 ** 31):
            w = O.philox_bits(seed, v, R.DRAW_VISIT, 2)[0]
            want = seed if v == 0 else int(w[0]) | (int(w[1]) << 32)
            assert RS.visit_seed(seed, v) == want == lib.mi_resample_visit_seed(seed, v), (seed, v)
    assert RS.DRAW_VISIT == 27 and (RS.DRAW_JUMP_L, RS.DRAW_JUMP_X, RS.DRAW_JUMP_T) == (24, 25, 26)
    used = [getattr(O, k) for k in dir(O) if k.startswith("DRAW_")]
    assert not set(range(24, 28)) & (set(used) | set(range(10, 24)))


# ---- the jump table -----------------------------------------------------------------------------------------------------------------

def _rel(got, want):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    return float(((got - want).abs() / want.abs().clamp_min(1e-300)).max())


@pytest.mark.parametrize("S", [None, 5])
@pytest.mark.parametrize("j", [1, 3])
def test_jump_table_is_consistent_with_the_forward_process(S, j):
    m = _module(20)
    v = m if S is None else m.respaced(S)
    T = v.beta_scheduler.timesteps
    ac, sig = (t.double() for t in (_tables(v)["alphas_cumprod"], _tables(v)["sigmas"]))
    t64 = RS.jump_table(v, j, dtype=torch.float64)
    assert t64.shape == (T + 1, 3) and torch.equal(t64, R.jump_table(_tables(v), j))
    a, b = torch.arange(0, T + 1 - j), torch.arange(j, T + 1)
    c0, c1, s = t64[a, 0], t64[a, 1], t64[a, 2]
    assert _rel(c0 * torch.sqrt(ac[a]), torch.sqrt(ac[b])) <= 1e-12                       # the signal of level b
    assert _rel(c0 ** 2 * (1 - ac[a]) + c1 ** 2, 1 - ac[b]) <= 1e-12                      # its noise variance
    assert _rel(sig[a] ** 2 + s ** 2, sig[b] ** 2) <= 1e-12                               # the coordinates' variance
    # a jump a -> a + 2 is two jumps of length 1 composed
    one, two = RS.jump_table(v, 1, dtype=torch.float64), RS.jump_table(v, 2, dtype=torch.float64)
    k = torch.arange(0, T - 1)
    assert _rel(one[k, 0] * one[k + 1, 0], two[k, 0]) <= 1e-12
    assert _rel(one[k + 1, 0] ** 2 * one[k, 1] ** 2 + one[k + 1, 1] ** 2, two[k, 1] ** 2) <= 1e-12
    assert _rel(one[k, 2] ** 2 + one[k + 1, 2] ** 2, two[k, 2] ** 2) <= 1e-12
    # the float32 table is the rounded float64 one, bit for bit; rows past T - j are zero
    t32 = RS.jump_table(v, j)
    assert t32.dtype == torch.float32 and torch.equal(t32, t64.float())
    assert bool((t32[T + 1 - j:] == 0).all()) and bool((t64[T + 1 - j:] == 0).all()) and bool((t32[:T + 1 - j, :2] > 0).all())
    for bad in (0, T + 1):
        with pytest.raises(ValueError):
            RS.jump_table(v, bad)


# ---- header and bindings ------------------------------------------------------------------------------------------------------------

def test_header_symbols_and_table():
    names = declared_symbols("matinvent_hip_resample.h")
    assert names == ["mi_batch_set_resampling", "mi_resample_jump", "mi_resample_schedule", "mi_resample_visit_seed"]
    assert sorted(_lib.RESAMPLE_SIGNATURES) == names and any(t is _lib.RESAMPLE_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    assert not set(names) & set(_lib.SIGNATURES)
    lib = _lib.load()
    for n in names:
        assert getattr(lib, n).argtypes == _lib.RESAMPLE_SIGNATURES[n][1] and getattr(lib, n).restype == _lib.RESAMPLE_SIGNATURES[n][0]


# ---- refusals without a GPU ---------------------------------------------------------------------------------------------------------

def test_library_refusals_on_the_host():
    lib = _lib.load()
    tab = np.ones((21, 3), dtype=np.float32)
    ptr = tab.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.mi_batch_set_resampling(None, ptr, 21, 3, 4) == _lib.MI_EINVAL and b"null handle" in lib.mi_last_error()
    assert lib.mi_batch_set_resampling(None, None, 0, 1, 0) == _lib.MI_EINVAL
    assert lib.mi_resample_jump(None, 1, 5, None, None, None, None) == _lib.MI_EINVAL
    for t_start, r, j in ((-1, 2, 2), (5, 0, 2), (5, 2, 0), (5, -3, 1)):
        assert lib.mi_resample_schedule(t_start, r, j, None, 0) == _lib.MI_EINVAL, (t_start, r, j)
        with pytest.raises(ValueError):
            RS.schedule(t_start, r, j)
    assert lib.mi_resample_schedule(5, 2, 2, None, 4) == _lib.MI_EINVAL      # a capacity without a buffer
    assert lib.mi_resample_schedule(0, 2, 2, None, 0) == 1                    # a chain that starts at level 0 visits it alone


def test_bad_r_j_n_are_refused_before_the_handle_is_touched():
    """mi_batch_set_resampling checks (n, r, j) and the table before it looks at the handle: the message names what was wrong."""
    lib = _lib.load()
    tab = np.ones((21, 3), dtype=np.float32)
    ptr = tab.ctypes.data_as(C.POINTER(C.c_float))
    for (n, r, j), msg in (((1, 2, 1), b"rows"), ((0, 2, 1), b"rows"), ((21, 0, 4), b"r = 0"), ((21, -1, 4), b"r = -1"), ((21, 3, 0), b"j = 0"),
                           ((21, 3, 21), b"j = 21"), ((21, 3, -2), b"j = -2")):
        assert lib.mi_batch_set_resampling(None, ptr, n, r, j) == _lib.MI_EINVAL and msg in lib.mi_last_error(), (n, r, j, lib.mi_last_error())
    for bad in (np.nan, np.inf):
        t2 = tab.copy()
        t2[7, 1] = bad
        assert lib.mi_batch_set_resampling(None, t2.ctypes.data_as(C.POINTER(C.c_float)), 21, 3, 4) == _lib.MI_EINVAL
        assert b"row 7" in lib.mi_last_error()
    assert lib.mi_batch_set_resampling(None, ptr, 21, 3, 20) == _lib.MI_EINVAL and b"null handle" in lib.mi_last_error()   # (valid arguments)
    for bad in ((0, 2), (2, 0), (2.5, 2), 3, (1, 2, 3)):
        with pytest.raises(ValueError):
            RS.check("sample", bad)
    assert RS.check("sample", None) is None and RS.check("sample", (2, 3)) == (2, 3) and RS.check("sample", [1, 1]) == (1, 1)


def test_value_errors_before_any_device_work(tmp_path):
    from matinvent_amd import pipeline, sampling
    from matinvent_amd.suite import DiffCSPSuite
    m = _module(20)
    c = Condition.composition("NaCl", 2)
    kw = dict(condition=c, resample=(2, 3))
    # (the module lives on the CPU: each refusal below comes before the call's first device work)
    for bad, match in ((dict(resample=(2, 3)), "condition"), (dict(kw, record=True), "record"), (dict(kw, noise={}), "noise"),
                       (dict(kw, likelihood="free"), "likelihood"), (dict(kw, t_stop=1), "t_stop"), (dict(condition=c, resample=(0, 3)), "r >= 1"),
                       (dict(condition=c, resample=(2, 0)), "j >= 1"), (dict(condition=c, resample=(2, 20)), "jump-off"),
                       (dict(kw, t_start=3), "jump-off"), (dict(condition=c, resample=(2, 21)), "jump-off")):
        with pytest.raises(ValueError, match=match):
            m.sample(c, **bad)
    with pytest.raises(ValueError, match="jump-off"):
        m.respaced(5).sample(c, condition=c, resample=(2, 5))
    with pytest.raises(ValueError, match="resample"):
        sampling.sample_mdp(2, None, resample=(2, 3))
    with pytest.raises(ValueError, match="resample"):
        sampling.sample_rollout(2, None, resample=(2, 3))
    s = sampling.DiffCSPSampler(batch_size=2, num_batches=1)
    with pytest.raises(ValueError, match="together"):
        s.generate(None, condition=c, resample_times=2)
    with pytest.raises(ValueError, match="need a condition"):
        s.generate(None, resample_times=2, jump_length=3)
    suite = DiffCSPSuite("diffcsp", {"batch_size": 4, "num_batches": 1}, {}, device="cpu")
    for key in ("resample_times", "jump_length"):
        with pytest.raises(ValueError, match=key):
            pipeline.MatInventPG(rl_epoch=1, model_suite=suite, reward=None, sample_cfg={key: 2}, finetune_cfg={}, save_dir=str(tmp_path),
                                 save_freq=1, device="cpu")
    # the pipelines' sample_cfg (MatInvent's and MatInventDPO's base) carries the keys to the sampler
    cfg = {"target_compositions_dict": [{"Na": 1, "Cl": 1}], "resample_times": 2, "jump_length": 5}
    rl = pipeline.ReinL(rl_epoch=1, model_suite=suite, reward=None, sample_cfg=cfg, finetune_cfg={}, save_dir=str(tmp_path), save_freq=1, device="cpu")
    assert rl.sample_cfg.resample_times == 2 and rl.sample_cfg.jump_length == 5
    assert issubclass(pipeline.MatInventDPO, pipeline.MatInvent) and pipeline.MatInventDPO.sample_step is pipeline.MatInvent.sample_step
