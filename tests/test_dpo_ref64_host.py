"""CPU-only checks that pin tests/dpo_ref64.py, the float64 reference of the preference micro-step: the closed-form gradient seeds against
float64 autograd of the total, the factorised d_b against the direct difference (equal in float64; in float32 the direct form cancels at
agent ~ prior and the factorised one does not), the overflow-free pair terms, and the boundary header with its ctypes table."""
import ctypes

import torch

from tests import dpo_ref64 as D
from tests import ft_ref64 as R

NA = [1, 2, 5, 3, 4]
PAIRS = [(0, 1), (2, 1), (0, 3), (3, 2)]          # crystal 0 wins twice, 1 loses twice, 2 and 3 both win and lose, 4 sits in no pair
BETA, P_GLOBAL, ACCUM = 50.0, 7, 3


def _draws(seed, spread):
    g = torch.Generator().manual_seed(seed)
    B, N = len(NA), sum(NA)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    pa = (r(B, 3, 3), r(N, 3), r(N, 100))
    pp = tuple(v + spread * r(*v.shape) for v in pa)
    q = lambda g_: tuple(v.float().double() for v in g_)   # float32 values, as a device's predictions are: the float32 runs see the same inputs
    return q(pa), q(pp), q((r(B, 3, 3), r(N, 3), r(N, 100)))


def test_seeds_match_float64_autograd_of_the_total():
    pa, pp, tg = _draws(0, 0.01)
    leaves = tuple(v.clone().requires_grad_(True) for v in pa)
    tot = D.total(leaves, pp, tg, D.COSTS, NA, PAIRS, BETA, P_GLOBAL, ACCUM)
    grads = torch.autograd.grad(tot, leaves)
    out = D.micro_step(pa, pp, tg, D.COSTS, NA, PAIRS, BETA, P_GLOBAL, ACCUM)
    for s, g in zip(out["seeds"], grads):
        assert float((s - g).abs().max()) <= 1e-14 * max(1.0, float(g.abs().max()))
    n2g = R._batch(NA)[1]
    assert float(out["coef"][4]) == 0.0 and all(torch.count_nonzero(s[n2g == 4] if s.shape[0] == sum(NA) else s[4]) == 0 for s in out["seeds"])
    assert float(out["coef"].abs().min()) == 0.0 and float(out["coef"][:4].abs().min()) > 0
    st = out["stats"]
    assert float(st[0]) == float(out["loss"].sum() / P_GLOBAL) and float(st[1]) == float((out["m"] < 0).sum()) and float(st[2]) == float(-out["m"].sum())


def test_factorised_delta_equals_the_direct_difference_in_float64_and_survives_float32():
    pa, pp, tg = _draws(1, 1e-4)
    ref = D.delta(pa, pp, tg, D.COSTS, NA)
    direct = D.delta_direct(pa, pp, tg, D.COSTS, NA)
    scale = float(ref.abs().max())
    L = D.sample_loss(pa, tg, D.COSTS, NA)
    assert float((ref - direct).abs().max()) <= 64 * 2.0 ** -52 * float(L.max())   # (float64's own cancellation: a few roundings of L ~ 40)
    assert scale < 1e-4 * float(L.max())
    fac32 = D.delta(pa, pp, tg, D.COSTS, NA, torch.float32).double()
    dir32 = D.delta_direct(pa, pp, tg, D.COSTS, NA, torch.float32).double()
    e_fac, e_dir = float((fac32 - ref).abs().max()) / scale, float((dir32 - ref).abs().max()) / scale
    assert e_fac <= 1e-5 and e_dir >= 100 * e_fac, (e_fac, e_dir)


def test_pair_terms_are_finite_and_exact_at_saturation():
    d = torch.tensor([0.0, 3.0, -5.0, 1e-9], dtype=torch.float64)
    m, u, loss, g = D.pair_terms(d, [(1, 0), (2, 0), (0, 1), (3, 0)], 200.0)
    assert m.tolist() == [3.0, -5.0, -3.0, 1e-9] and u[:3].tolist() == [600.0, -1000.0, -600.0] and abs(float(u[3]) - 2e-7) < 1e-20
    assert bool(torch.isfinite(loss).all() and torch.isfinite(g).all())
    assert float(loss[0]) == 600.0 and float(loss[1]) == 0.0 and float(g[0]) == 1.0 and float(g[1]) == 0.0
    assert abs(float(loss[3]) - (0.6931471805599453 + 1e-7)) < 1e-12 and abs(float(g[3]) - 0.5) < 1e-7
    x = u.clone().requires_grad_(True)
    torch.nn.functional.softplus(x[3:]).sum().backward()
    assert abs(float(x.grad[3]) - float(g[3])) < 1e-15              # d softplus / du = sigmoid


def test_dpo_header_is_exported_and_bound_in_its_own_table():
    from matinvent_amd import _lib
    from matinvent_amd.build import build
    from tests.header_util import declared_symbols
    names = declared_symbols("matinvent_hip_dpo.h")
    assert sorted(names) == ["mi_batch_num_pairs", "mi_batch_set_pairs", "mi_dpo_micro_step"]
    lib = ctypes.CDLL(build(verbose=False))
    assert all(hasattr(lib, n) for n in names)
    assert sorted(_lib.DPO_SIGNATURES) == sorted(names) and any(t is _lib.DPO_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    assert not set(names) & set(_lib.SIGNATURES)
    bound = _lib.load()
    for n in names:
        assert getattr(bound, n).argtypes == _lib.DPO_SIGNATURES[n][1] and getattr(bound, n).restype == _lib.DPO_SIGNATURES[n][0]
    assert len(_lib.DPO_SIGNATURES["mi_dpo_micro_step"][1]) == 31
    # refused on the host, before any device work: null handles
    assert bound.mi_batch_set_pairs(None, None, None, 0) == _lib.MI_EINVAL and b"null handle" in bound.mi_last_error()
    assert bound.mi_batch_num_pairs(None) == 0
    z = [None] * 9
    assert bound.mi_dpo_micro_step(*z, 1, 1.0, 0.0, 0.1, 1.0, 0, 1, None, None, None, 1.0, 1.0, 20.0, 1.0, 1, 1, None, None, None, None, None,
                                   None) == _lib.MI_EINVAL
