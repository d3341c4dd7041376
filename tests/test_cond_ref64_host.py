"""CPU checks of the conditioning layer that needs no GPU: tests/cond_ref64.py (the float64 restatement the GPU tests compare the
kernel with) against an element-by-element evaluation of the three formulas, its mask handling, its exact level-0 branch and its
independence from crystal order and offsets; Condition's bookkeeping (composition, template, slice); the new header's symbols and the
host-side refusals."""
import numpy as np
import pytest
import torch

from matinvent_amd import _lib
from matinvent_amd.conditioning import Condition, composition_types, parse_composition
from matinvent_amd.structure import SYMBOLS, reduced_formula
from oracle import diffcsp_oracle as O
from tests import cond_ref64 as R
from tests.header_util import declared_symbols

NA = [1, 4, 5, 2]
SEED = 77
T = 20


def _tables():
    g = torch.Generator().manual_seed(5)
    ac = torch.cat([torch.ones(1), torch.sort(torch.rand(T, generator=g), descending=True).values]).float()
    sig = torch.cat([torch.zeros(1), torch.sort(0.005 + 0.5 * torch.rand(T, generator=g)).values]).float()
    return dict(alphas_cumprod=ac, sigmas=sig)


def _cond(na, seed, mode="mixed"):
    g = torch.Generator().manual_seed(seed)
    B, N = len(na), sum(na)
    pick = {"all": lambda n: torch.ones(n, dtype=torch.bool), "none": lambda n: torch.zeros(n, dtype=torch.bool),
            "mixed": lambda n: torch.rand(n, generator=g) < 0.5}[mode]
    return Condition(na, atom_types=torch.randint(1, 101, (N,), generator=g), known_types=pick(N),
                     frac_coords=torch.rand(N, 3, generator=g), known_coords=pick(N),
                     lattices=4 * torch.randn(B, 3, 3, generator=g), known_lattice=pick(B))


def _state(na, seed):
    g = torch.Generator().manual_seed(seed)
    B, N = len(na), sum(na)
    return torch.randn(N, 100, generator=g), torch.rand(N, 3, generator=g), torch.randn(B, 3, 3, generator=g)


def test_draw_ids_extend_the_contract_without_a_collision():
    used = [getattr(O, k) for k in dir(O) if k.startswith("DRAW_")]
    new = [R.DRAW_COND_L, R.DRAW_COND_X, R.DRAW_COND_T]
    assert new == [21, 22, 23] and not set(new) & set(used) and not set(new) & set(range(10, 21))


def test_impose_is_the_three_formulas_element_by_element():
    c, st, tab = _cond(NA, 1), _state(NA, 2), R.level_table(_tables())
    level = 7
    z = R.draws(SEED, level, NA, node_offset=11, graph_offset=3)
    # the draws are the contract's: element (node_offset + i) * width + column of draw 21 / 22 / 23 at step = level
    assert float(z[2][2, 5]) == float(O.philox_normal(SEED, level, 23, 1, (11 + 2) * 100 + 5)[0])
    assert float(z[1][4, 1]) == float(O.philox_normal(SEED, level, 22, 1, (11 + 4) * 3 + 1)[0])
    assert float(z[0][1, 2, 0]) == float(O.philox_normal(SEED, level, 21, 1, (3 + 1) * 9 + 6)[0])
    a, x, l = R.impose(st, c, tab, level, z)
    c0, c1, sig = (float(v) for v in tab[level])
    for i in range(sum(NA)):
        for k in range(100):
            want = c0 * (1.0 if int(c.atom_types[i]) - 1 == k else 0.0) + c1 * float(z[2][i, k]) if c.known_types[i] else float(st[0][i, k])
            assert float(a[i, k]) == want
        for k in range(3):
            want = (float(c.frac_coords[i, k]) + sig * float(z[1][i, k])) % 1.0 if c.known_coords[i] else float(st[1][i, k])
            assert float(x[i, k]) == want
    for b in range(len(NA)):
        for k in range(9):
            want = c0 * float(c.lattices.view(-1, 9)[b, k]) + c1 * float(z[0].view(-1, 9)[b, k]) if c.known_lattice[b] else float(st[2].view(-1, 9)[b, k])
            assert float(l.view(-1, 9)[b, k]) == want


@pytest.mark.parametrize("mode", ["all", "none", "mixed"])
def test_masks_and_the_exact_level_zero_branch(mode):
    c, st, tab = _cond(NA, 3, mode), _state(NA, 4), R.level_table(_tables())
    for level in (0, 1, T):
        z = R.draws(SEED, level, NA)
        a, x, l = R.impose(st, c, tab, level, z, dtype=torch.float32)
        assert torch.equal(a[~c.known_types], st[0][~c.known_types]) and torch.equal(x[~c.known_coords], st[1][~c.known_coords])
        assert torch.equal(l[~c.known_lattice], st[2][~c.known_lattice])
        if mode == "none":
            assert all(torch.equal(u, v) for u, v in zip((a, x, l), st))
        if level == 0:   # the clean values themselves, whatever the table holds
            garbage = torch.full_like(tab, float("nan"))
            a0, x0, l0 = R.impose(st, c, garbage, 0, z, dtype=torch.float32)
            assert torch.equal(a0, a) and torch.equal(x0, x) and torch.equal(l0, l)
            assert torch.equal(l[c.known_lattice], c.lattices[c.known_lattice]) and torch.equal(x[c.known_coords], c.frac_coords[c.known_coords])
            rows = a[c.known_types]
            assert torch.equal(rows.argmax(dim=1) + 1, c.atom_types[c.known_types]) and set(rows.unique().tolist()) <= {0.0, 1.0}
            assert bool((rows.sum(dim=1) == 1).all())
        elif mode == "all":
            assert not torch.equal(a, st[0]) and not torch.equal(l, st[2])


def test_independent_of_crystal_grouping_and_offsets():
    """A sub-batch imposed with its global offsets gives the rows of the whole batch (what makes split batches and shards agree)."""
    c, st, tab = _cond(NA, 5, "all"), _state(NA, 6), R.level_table(_tables())
    level, no, go = 9, 1000003, 4099
    whole = R.impose(st, c, tab, level, R.draws(SEED, level, NA, no, go))
    g0, n0 = 2, sum(NA[:2])
    part = R.impose((st[0][n0:], st[1][n0:], st[2][g0:]), c.slice(g0, len(NA)), tab, level, R.draws(SEED, level, NA[g0:], no + n0, go + g0))
    assert torch.equal(part[0], whole[0][n0:]) and torch.equal(part[1], whole[1][n0:]) and torch.equal(part[2], whole[2][g0:])
    other = R.impose((st[0][n0:], st[1][n0:], st[2][g0:]), c.slice(g0, len(NA)), tab, level, R.draws(SEED, level, NA[g0:], no, go))
    assert not torch.equal(other[0], whole[0][n0:])


def test_composition_bookkeeping():
    targets = [{"Li": 2, "O": 1}, {"Na": 1, "Cl": 1}]
    c = Condition.composition(targets, 5)
    assert c.num_atoms.tolist() == [3, 2, 3, 2, 3] and len(c) == 5 and c.num_nodes == 13
    assert c.atom_types.tolist() == [3, 3, 8, 11, 17] * 2 + [3, 3, 8]            # ordered by atomic number, cycling through the list
    assert bool(c.known_types.all()) and not bool(c.known_coords.any()) and not bool(c.known_lattice.any())
    assert [SYMBOLS[z] for z in composition_types("LiFePO4")] == ["Li", "O", "O", "O", "O", "P", "Fe"]
    assert parse_composition("Li2O") == {"Li": 2, "O": 1} and composition_types({"O": 1, "Li": 2}) == [3, 3, 8]
    one = Condition.composition("SiO2", 2)
    assert one.num_atoms.tolist() == [3, 3] and reduced_formula(one.atom_types[:3].tolist()) == "O2Si"
    for bad in ("li2O", "Li2O)", {"Xx": 1}, {"Li": -1}, {}, {"Li": 1.5}):
        with pytest.raises(ValueError):
            Condition.composition(bad, 1)
    s = c.slice(1, 4)
    assert s.num_atoms.tolist() == [2, 3, 2] and s.atom_types.tolist() == [11, 17, 3, 3, 8, 11, 17] and bool(s.known_types.all())
    assert len(c.slice(2, 2)) == 0


def test_template_bookkeeping():
    from matinvent_amd.data import CrystalData, lattice_params_to_matrix
    d = CrystalData(torch.tensor([[0.0, 0.5, 0.25], [0.1, 0.2, 0.3], [0.9, 0.8, 0.7]]), torch.tensor([3, 8, 3]), torch.tensor([[4.0, 5.0, 6.0]]),
                    torch.tensor([[90.0, 80.0, 70.0]]))
    t = Condition.template(d, 2, types=[True, False, True], coords=True, lattice=True)
    assert t.num_atoms.tolist() == [3, 3] and t.atom_types.tolist() == [3, 8, 3] * 2
    assert t.known_types.tolist() == [True, False, True] * 2 and bool(t.known_coords.all()) and t.known_lattice.tolist() == [True, True]
    assert torch.equal(t.frac_coords, d.frac_coords.repeat(2, 1))
    assert torch.equal(t.lattices[1], lattice_params_to_matrix(d.lengths, d.angles)[0])
    u = Condition.template(d, 3)                                      # the default: every type, nothing else
    assert bool(u.known_types.all()) and not bool(u.known_coords.any()) and not bool(u.known_lattice.any())
    w = Condition.template(d, 1, types=False, coords=[False, True, False])
    assert w.known_coords.tolist() == [False, True, False] and not bool(w.known_types.any())
    with pytest.raises(ValueError):
        Condition.template(d, 1, coords=[True, False])
    s = t.slice(1, 2)
    assert s.num_atoms.tolist() == [3] and torch.equal(s.lattices, t.lattices[1:]) and s.known_types.tolist() == [True, False, True]
    with pytest.raises(ValueError):
        Condition([2], atom_types=[0, 5], known_types=[True, True])
    with pytest.raises(ValueError):
        Condition([2], atom_types=[1, 2, 3], known_types=[True, True, True])
    with pytest.raises(ValueError):
        Condition([2], known_coords=[True, False])


def test_header_symbols_and_table():
    names = declared_symbols("matinvent_hip_cond.h")
    assert names == ["mi_batch_set_condition", "mi_condition_apply"] and sorted(_lib.COND_SIGNATURES) == names
    assert any(t is _lib.COND_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    assert [f for f, _ in _lib.Condition._fields_] == ["known_types_host", "known_coords_host", "known_lattice_host", "types0_host",
                                                       "frac0_host", "lat0_host"]


def test_host_side_refusals(tmp_path):
    from matinvent_amd import pipeline, sampling
    from matinvent_amd.suite import DiffCSPSuite
    c = Condition.composition("NaCl", 2)
    with pytest.raises(ValueError, match="condition"):
        sampling.sample_mdp(2, None, condition=c)
    with pytest.raises(ValueError, match="condition"):
        sampling.sample_rollout(2, None, condition=c)
    with pytest.raises(ValueError, match="not both"):
        sampling.DiffCSPSampler(batch_size=2, num_batches=1).generate(None, condition=c, target_compositions_dict=[{"Na": 1}])
    with pytest.raises(ValueError, match="covers 2 crystals"):
        sampling.DiffCSPSampler(batch_size=3, num_batches=1).generate(None, condition=c)
    suite = DiffCSPSuite("diffcsp", {"batch_size": 4, "num_batches": 1}, {}, device="cpu")
    with pytest.raises(ValueError, match="target_compositions_dict"):
        pipeline.MatInventPG(rl_epoch=1, model_suite=suite, reward=None, sample_cfg={"target_compositions_dict": [{"Na": 1, "Cl": 1}]},
                             finetune_cfg={}, save_dir=str(tmp_path), save_freq=1, device="cpu")
    # MatInvent's sample_cfg carries the key to the sampler
    rl = pipeline.ReinL(rl_epoch=1, model_suite=suite, reward=None, sample_cfg={"target_compositions_dict": [{"Na": 1, "Cl": 1}]},
                        finetune_cfg={}, save_dir=str(tmp_path), save_freq=1, device="cpu")
    assert [dict(d) for d in rl.sample_cfg.target_compositions_dict] == [{"Na": 1, "Cl": 1}]
