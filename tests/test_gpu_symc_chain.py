"""GPU checks of the symmetry-constrained reverse chain (DiffCSPModule.sample(symmetry=), mi_sampler_run's hook) on the
64-wide, 2-layer network of tests/test_gpu_respaced_chain.py with T = 20 and chains of at most 8 steps:

1. a constrained chain IS unconstrained single steps with mi_symmetry_apply between them, bit for bit -- on the full grid and on a view,
   with and without a condition on the atom types, and on two streams;
2. a constraint of the identity everywhere is the plain chain, bit for bit, and a used handle carries nothing into the next call;
3. the final states of rutile- and rock-salt-templated batches meet the CPU certificates of tests/symc_ref64.py;
4. with symmetry_fix_types the final species are the template's;
5. what is refused."""
import numpy as np
import pytest
import torch

import tests.test_gpu_respaced_chain as RC
from matinvent_amd import _lib, conditioning
from matinvent_amd import symmetry_constraint as SC
from matinvent_amd.cspnet import _ptr, _stream
from matinvent_amd.data import SimpleStructure
from tests import refine_ref64 as RR
from tests import symc_cases as CS
from tests import symc_ref64 as V
from tests.gpu_util import Box

pytestmark = pytest.mark.gpu

T = 20
STEP_LR = RC.STEP_LR
STATE = ("atom_types", "frac_coords", "lattices")


@pytest.fixture(scope="module")
def base():
    return RC._base()[0]


def mixed():
    """Rutile, a free crystal of three atoms, the P-1 pair, rock salt: constrained and free crystals in one batch."""
    return SC.stack([CS.constraint("rutile"), SC.SymmetryConstraint.identity([3], atom_types=[3, 8, 8]), CS.constraint("p1bar_pair"), CS.constraint("rocksalt_conv")])


def record_of(name):
    L, z, f = CS.crystal(name)
    p = RR.cell_parameters(L)
    return SimpleStructure(p[:3], p[3:], [int(v) for v in z], np.asarray(f, np.float64))


@pytest.mark.parametrize("with_condition", [False, True])
@pytest.mark.parametrize("S", [None, 5])
def test_constrained_chain_is_single_steps_plus_projections(base, S, with_condition):
    v = base if S is None else base.respaced(S)
    Tv = v.beta_scheduler.timesteps
    steps = min(6, Tv)
    c = mixed()
    na = [int(n) for n in c.num_atoms]
    cond = c.condition(types=True) if with_condition else None
    seed = 56
    final, traj, info = v.sample(c, step_lr=STEP_LR, seed=seed, streams=1, t_start=steps, symmetry=c, condition=cond)
    assert sorted(traj) == [0] and info["cell_failures"].tolist() == [0] * len(c)
    lib = _lib.load()
    cb = v.make_batch(na)
    c.attach(cb)
    if cond is not None:
        cond.attach(v, cb)
    N, B = sum(na), len(na)
    x, l, a = torch.empty(N, 3, device="cuda"), torch.empty(B, 3, 3, device="cuda"), torch.empty(N, 100, device="cuda")
    _lib.check(lib.mi_sampler_init_state(cb._h, seed, Tv, _ptr(a), _ptr(x), _ptr(l), _stream()))
    if cond is not None:
        conditioning.apply(cb, steps, seed, a, x, l)
    SC.apply(cb, a, x, l)
    cur = dict(atom_types=a, frac_coords=x, lattices=l)
    box = Box(na)
    for t in range(steps, 0, -1):
        f, _ = v.sample(box, step_lr=STEP_LR, seed=seed, streams=1, init=(cur["frac_coords"], cur["lattices"], cur["atom_types"]), t_start=t, t_stop=t - 1)
        if cond is not None:
            conditioning.apply(cb, t - 1, seed, f["atom_types"], f["frac_coords"], f["lattices"])
        SC.apply(cb, f["atom_types"], f["frac_coords"], f["lattices"])
        cur = {k: f[k] for k in STATE}
    for k in STATE:
        assert torch.equal(final[k], cur[k]), k
    assert SC.failures(cb).tolist() == [0] * B
    SC.SymmetryConstraint.clear(cb)
    if cond is not None:
        conditioning.Condition.clear(cb)
        assert torch.equal(final["atom_types"].argmax(1).cpu() + 1, c.atom_types)   # level 0: the template's species exactly
    # the constrained chain is not the plain one, and every state it ends in carries its group
    plain, _ = v.sample(box, step_lr=STEP_LR, seed=seed, streams=1, t_start=steps)
    assert not torch.equal(plain["frac_coords"], final["frac_coords"])
    xs, ls, ts = (final[k].cpu().numpy() for k in ("frac_coords", "lattices", "atom_types"))
    for i in range(B):
        lo, hi = sum(na[:i]), sum(na[:i + 1])
        assert V.coordinate_defect(c, i, xs[lo:hi]) <= 1.0 and V.cell_defect(c, i, ls[i]) <= 1.0 and V.orbits_share_rows(c, i, ts[lo:hi]), i


@pytest.mark.parametrize("S", [None, 7])
def test_two_streams_are_the_two_groups_one_after_the_other(base, S):
    v = base if S is None else base.respaced(S)
    c = SC.stack([mixed(), mixed().select([3, 2, 1, 0])])
    na = [int(n) for n in c.num_atoms]
    kw = dict(step_lr=STEP_LR, seed=57, t_start=4)
    two = v.sample(Box(na), streams=2, symmetry=c, **kw)
    h = len(na) // 2
    n0 = sum(na[:h])
    seq = [v.sample(Box(na[:h]), streams=1, symmetry=c.slice(0, h), **kw),
           v.sample(Box(na[h:]), streams=1, node_offset=n0, graph_offset=h, symmetry=c.slice(h, len(na)), **kw)]
    for k in STATE:
        assert torch.equal(torch.cat([s_[0][k] for s_ in seq]), two[0][k]), k
    assert two[2]["cell_failures"].tolist() == [0] * len(na) and len(seq[0][2]["cell_failures"]) == h


def test_the_identity_everywhere_is_the_plain_chain_and_a_used_handle_is_clean(base):
    na = [1, 3, 7]
    box = Box(na)
    kw = dict(step_lr=STEP_LR, seed=58, streams=1, t_start=4)
    never = base.sample(box, **kw)
    ident = base.sample(box, symmetry=SC.SymmetryConstraint.identity(na), **kw)
    assert len(ident) == 3 and ident[2]["cell_failures"].tolist() == [0, 0, 0]
    for k in STATE:
        assert torch.equal(ident[0][k], never[0][k]), k
    c = SC.stack([CS.constraint("one_atom_cubic"), SC.SymmetryConstraint.identity([3]), SC.SymmetryConstraint.identity([7])])
    con = base.sample(box, symmetry=c, **kw)                  # the same cached handle, constrained ...
    assert not torch.equal(con[0]["frac_coords"], never[0]["frac_coords"]) and float(con[0]["frac_coords"][0].abs().max()) == 0.0
    again = base.sample(box, **kw)                            # ... and not any more
    assert len(again) == 2
    for k in STATE:
        assert torch.equal(again[0][k], never[0][k]), k


@pytest.mark.parametrize("name", ["rutile", "rocksalt_conv"])
def test_a_templated_batch_meets_the_certificates(base, name):
    c = SC.SymmetryConstraint.template(record_of(name), 3)
    assert c.num_ops == [CS.EXPECTED_OPS[name]] * 3 and c.atom_types.tolist() == [int(v) for v in CS.crystal(name)[1]] * 3
    assert sorted(np.bincount(c.parts[0].rep).tolist()) == sorted(np.bincount(CS.constraint(name).parts[0].rep).tolist())   # the Wyckoff multiplicities
    final, _, info = base.sample(c, step_lr=STEP_LR, seed=59, streams=1, t_start=8, symmetry=c)
    assert info["cell_failures"].tolist() == [0, 0, 0]
    n = int(c.num_atoms[0])
    xs, ls, ts = (final[k].cpu().numpy() for k in ("frac_coords", "lattices", "atom_types"))
    worst = [0.0, 0.0]
    for i in range(3):
        worst = [max(worst[0], V.coordinate_defect(c, i, xs[i * n:(i + 1) * n])), max(worst[1], V.cell_defect(c, i, ls[i]))]
        assert V.orbits_share_rows(c, i, ts[i * n:(i + 1) * n])
    print(f"{name}: coordinate defect {worst[0]:.3f}, cell defect {worst[1]:.3f} (each in units of its bound)")
    assert worst[0] <= 1.0 and worst[1] <= 1.0
    assert not np.array_equal(xs[:n], xs[n:2 * n]) or name == "rocksalt_conv"    # (every rock-salt coordinate is fixed)


def test_generate_with_a_template_and_fixed_types(base, tmp_path):
    import json
    from matinvent_amd.sampling import DiffCSPSampler
    rec = record_of("rutile")
    s = DiffCSPSampler(seed=5)
    data, strucs = s.generate(base, batch_size=3, num_batches=1, sample_steps=5, symmetry_template=rec, symmetry_fix_types=True)
    assert len(data) == len(strucs) == 3 and s.last_symmetry["cell_failures"].tolist() == [0, 0, 0]
    assert all(d.atom_types.tolist() == [int(v) for v in rec.species] for d in data)
    path = tmp_path / "rutile.json"
    path.write_text(json.dumps(dict(lengths=list(rec.lengths), angles=list(rec.angles), species=list(rec.species), frac_coords=rec.frac_coords.tolist())))
    data2, _ = DiffCSPSampler(seed=5).generate(base, batch_size=3, num_batches=1, sample_steps=5, symmetry_template=str(path))
    assert [d.num_atoms for d in data2] == [6, 6, 6]
    for d in data2:   # the species are free but shared inside the orbits (2 + 4)
        z = d.atom_types.tolist()
        assert len(set(z[:2])) == 1 and len(set(z[2:])) == 1


def test_refusals(base):
    from matinvent_amd import pipeline, sampling
    from matinvent_amd.suite import DiffCSPSuite
    c = SC.stack([CS.constraint("rutile")])
    with pytest.raises(ValueError, match="symmetry"):
        sampling.sample_rollout(1, base, symmetry=c)
    with pytest.raises(ValueError, match="symmetry"):
        sampling.sample_mdp(1, base, symmetry=c)
    suite = DiffCSPSuite("diffcsp", {"batch_size": 4, "num_batches": 1}, {}, device="cpu")
    with pytest.raises(ValueError, match="sample_cfg.symmetry_template"):
        pipeline.MatInventPG(rl_epoch=1, model_suite=suite, reward=None, sample_cfg={"symmetry_template": "/x.json"}, finetune_cfg={}, save_dir="/tmp", save_freq=1,
                             device="cpu")
    # the library refuses, before anything is enqueued, what the keyword checks of sample() cannot see: a handle that carries a constraint
    cb = base.make_batch([6])
    c.attach(cb)
    kw = dict(step_lr=STEP_LR, seed=60, streams=1, t_start=2)
    with pytest.raises(_lib.MIError, match="records") as e:
        base.sample(cb, record=True, **kw)
    assert e.value.code == _lib.MI_EINVAL
    known = conditioning.Condition([6], atom_types=[int(z) for z in CS.crystal("rutile")[1]], known_types=[True] * 6, frac_coords=np.zeros((6, 3)), known_coords=[True] + [False] * 5)
    known.attach(base, cb)
    with pytest.raises(_lib.MIError, match="coordinate or a lattice") as e:
        base.sample(cb, **kw)
    assert e.value.code == _lib.MI_EINVAL
    conditioning.Condition.clear(cb)
    final, _ = base.sample(cb, **kw)                          # the handle's constraint still works
    assert V.coordinate_defect(c, 0, final["frac_coords"].cpu().numpy()) <= 1.0
    SC.SymmetryConstraint.clear(cb)
