"""CPU checks of symmetry-constrained sampling that need no GPU (matinvent_amd.symmetry_constraint, include/matinvent_hip_symc.h; DESIGN
57): the four certificates of a projected state under the float64 restatement (tests/symc_ref64.py) on the chain's starting point, the
identity's bits, from_operations' refusals, slice / select / stack, the kernel's order run on the host under the sanitizers, the header
with its table and build list, and every keyword refusal by name."""
import os
import shutil
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from matinvent_amd import _lib
from matinvent_amd import symmetry_constraint as SC
from tests import symc_cases as CS
from tests import symc_ref64 as V
from tests.header_util import ROOT, declared_symbols

TRIALS = 4


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def mod1(d):
    d = np.abs(d.astype(np.float64))
    return np.minimum(d, 1.0 - d)


@pytest.mark.parametrize("name", CS.NAMES)
def test_constraint_of_the_known_crystals(name):
    c = CS.constraint(name)
    p = c.parts[0]
    assert c.num_ops == [CS.EXPECTED_OPS[name]] and len(c) == 1 and c.num_nodes == len(CS.crystal(name)[1])
    assert (p.rep[p.rep] == p.rep).all() and (p.rep <= np.arange(p.n)).all()
    assert all(p.sigma[p.kof[j], p.rep[j]] == j for j in range(p.n))
    if name == "one_atom_cubic":   # every coordinate is fixed: P = 0
        assert np.abs(p.Q).max() == 0.0 and np.abs(p.d - np.round(p.d)).max() < 1e-15
    if name == "wurtzite":         # sites on the three-fold axis: thirds in d
        xy = p.d[:, :2]
        assert np.abs(xy * 3.0 - np.round(xy * 3.0)).max() < 1e-12 and np.abs(xy - np.round(xy)).min() > 0.3
        assert np.abs(p.Q.reshape(-1, 3, 3)[:, :, :2]).max() == 0.0   # only z is free
    if name == "rocksalt_conv":
        assert len(p.distinct) == 48 and sorted(set(int(v) for v in p.rep)) == [0, 4]
    if name == "p1bar_171":
        assert len(set(int(v) for v in p.rep)) == 86


@pytest.mark.parametrize("name", CS.NAMES)
def test_projected_random_states_meet_the_four_certificates(name):
    c = CS.constraint(name)
    na = [int(v) for v in c.num_atoms]
    rng = np.random.default_rng(560 + CS.NAMES.index(name))
    worst = [0.0, 0.0, 0.0]
    for _ in range(TRIALS):
        a, x, l = V.random_state(rng, na)
        a2, x2, l2, fail = V.project(c, a, x, l)
        assert x2.dtype == np.float32 and (x2 >= 0).all() and (x2 < 1).all()
        worst[0] = max(worst[0], V.coordinate_defect(c, 0, x2))                      # 1. the coordinate certificate
        if fail[0] == 0:
            worst[1] = max(worst[1], V.cell_defect(c, 0, l2[0]))                     # 2. the cell residual
            assert l2[0][1] == l2[0][2] == l2[0][5] == 0 and l2[0][0] > 0 and l2[0][4] > 0 and l2[0][8] > 0
        else:
            assert np.array_equal(bits(l2), bits(l))
        assert V.orbits_share_rows(c, 0, a2)                                         # 3. the types
        a3, x3, l3, _ = V.project(c, a2, x2, l2)                                     # 4. idempotence
        worst[2] = max(worst[2], float(mod1(x3 - x2).max()) / 2.0 ** -24)
        assert np.array_equal(bits(a3), bits(a2))
    print(f"{name}: coordinate defect {worst[0]:.3f}, cell defect {worst[1]:.3f}, second projection {worst[2]:.3f} (each in units of its bound)")
    assert worst[0] <= 1.0 and worst[1] <= 1.0 and worst[2] <= 1.0


def test_identity_keeps_every_bit_and_mixes_with_constrained_crystals():
    rs = CS.constraint("rocksalt_conv")
    c = SC.stack([SC.SymmetryConstraint.identity([3, 5]), rs, SC.SymmetryConstraint.identity([2])])
    assert [int(v) for v in c.num_atoms] == [3, 5, 8, 2] and c.num_ops == [1, 1, 192, 1]
    rng = np.random.default_rng(7)
    a, x, l = V.random_state(rng, [3, 5, 8, 2])
    x[0, 0], l[3, 4] = np.float32(-0.25), np.float32("nan")   # a free crystal is not even wrapped
    a2, x2, l2, fail = V.project(c, a, x, l)
    free = np.r_[0:8, 16:18]
    assert np.array_equal(bits(a2[free]), bits(a[free])) and np.array_equal(bits(x2[free]), bits(x[free]))
    assert np.array_equal(bits(l2[[0, 1, 3]]), bits(l[[0, 1, 3]])) and fail.tolist() == [0, 0, 0, 0]
    assert not np.array_equal(x2[8:16], x[8:16]) and V.coordinate_defect(c, 2, x2[8:16]) <= 1.0


def test_slice_select_stack():
    c = SC.stack([CS.constraint("rutile"), SC.SymmetryConstraint.identity([4]), CS.constraint("wurtzite"), CS.constraint("p1bar_pair")])
    assert len(c) == 4 and c.num_nodes == 6 + 4 + 4 + 2 and c.atom_types is None
    s = c.slice(1, 3)
    assert [int(v) for v in s.num_atoms] == [4, 4] and s.num_ops == [1, 12]
    q = c.select([3, 0])
    assert q.num_ops == [2, 16] and q.atom_types.tolist() == [14, 14] + list(CS.crystal("rutile")[1])
    a = c.arrays()
    assert a["op_off"].tolist() == [0, 16, 17, 29, 31] and a["distinct_off"].tolist() == [0, 16, 17, 29, 31] and a["rot"].shape == (31, 9)
    assert a["rep"].shape == (16,) and a["Q"].shape == (16, 9) and a["d"].shape == (16, 3) and a["Q"].dtype == np.float64 and a["rep"].dtype == np.int32
    two = SC.stack([q, s])
    assert two.num_ops == [2, 16, 1, 12]
    copies = SC.SymmetryConstraint.from_operations(6, CS.crystal("rutile")[2], *CS.operations("rutile"), tol=1e-6, atom_types=CS.crystal("rutile")[1], copies=3)
    assert len(copies) == 3 and copies.num_ops == [16] * 3 and copies.orbit.tolist() == CS.constraint("rutile").orbit.tolist() * 3


def test_condition_of_the_template():
    from matinvent_amd.conditioning import Condition
    c = SC.stack([CS.constraint("rutile")] * 2)
    cond = c.condition(types=True)
    assert cond.known_types.all() and not cond.known_coords.any() and not cond.known_lattice.any()
    assert cond.atom_types.tolist() == list(CS.crystal("rutile")[1]) * 2
    z = list(CS.crystal("rutile")[1]) * 2
    bad = list(z)
    bad[3] = 9   # one oxygen of an orbit of four
    with pytest.raises(ValueError, match="orbit"):
        c.check_condition(Condition([6, 6], atom_types=bad, known_types=[True] * 12))
    with pytest.raises(ValueError, match="orbit"):
        c.check_condition(Condition([6, 6], atom_types=z, known_types=[True] * 3 + [False] + [True] * 8))
    with pytest.raises(ValueError, match="coordinate or a lattice"):
        c.check_condition(Condition([6, 6], atom_types=z, known_types=[True] * 12, frac_coords=np.zeros((12, 3)), known_coords=[True] + [False] * 11))
    with pytest.raises(ValueError, match="atom counts"):
        c.check_condition(Condition([6], atom_types=z[:6], known_types=[True] * 6))
    with pytest.raises(ValueError, match="no template atom types"):
        SC.stack([c, SC.SymmetryConstraint.identity([2])]).condition()


def test_from_operations_refuses_by_name():
    L, z, f = CS.crystal("rutile")
    W, t = CS.operations("rutile")
    F = SC.SymmetryConstraint.from_operations
    with pytest.raises(ValueError, match="not a group"):          # a subset that is not closed
        F(6, f, W[:5], t[:5], tol=1e-6)
    with pytest.raises(ValueError, match="not a group"):          # a translation that no product gives
        thirds = np.array([[0.0, 0, 0], [1.0 / 3.0, 0, 0], [2.0 / 3.0, 0, 0]])
        F(3, thirds, np.tile(np.eye(3, dtype=int), (2, 1, 1)), thirds[:2], tol=1e-6)
    with pytest.raises(ValueError, match="broken site map"):      # an atom moved off its site
        f2 = f.copy()
        f2[4] += [0.03, 0.0, 0.0]
        F(6, f2, W, t, tol=1e-3)
    with pytest.raises(ValueError, match="broken site map"):      # maps confined to species: an oxygen relabelled
        F(6, f, W, t, tol=1e-3, atom_types=[22, 22, 8, 8, 8, 9])
    with pytest.raises(ValueError, match="det W"):
        W2 = W.copy()
        W2[1] = [[2, 0, 0], [0, 1, 0], [0, 0, 1]]
        F(6, f, W2, t, tol=1e-3)
    with pytest.raises(ValueError, match="cap of 192"):
        F(1, np.zeros((1, 3)), np.tile(np.eye(3, dtype=int), (193, 1, 1)), np.zeros((193, 3)))
    with pytest.raises(ValueError, match="cap of 256"):
        F(257, np.random.default_rng(0).uniform(0, 1, (257, 3)), np.stack([np.eye(3, dtype=int), -np.eye(3, dtype=int)]), np.zeros((2, 3)))
    with pytest.raises(ValueError, match="identity"):
        F(2, f[:2], -np.eye(3, dtype=int).reshape(1, 3, 3), np.zeros((1, 3)))
    with pytest.raises(ValueError, match="integers"):
        F(2, f[:2], np.eye(3).reshape(1, 3, 3) * 0.5, np.zeros((1, 3)))
    big = F(300, np.random.default_rng(0).uniform(0, 1, (300, 3)), np.eye(3, dtype=int).reshape(1, 3, 3), np.zeros((1, 3)))   # the identity has no atom cap
    assert big.num_ops == [1]


def test_translations_with_small_defects_are_closed_by_the_average():
    """from_operations averages the closure defects out of the translations: a list that closes to 1e-7 closes to rounding afterwards."""
    L, z, f = CS.crystal("rutile")
    W, t = CS.operations("rutile")
    rng = np.random.default_rng(3)
    c = SC.SymmetryConstraint.from_operations(6, f, W, t + rng.uniform(-1e-7, 1e-7, t.shape), tol=1e-5, atom_types=z)
    _, t2, _ = c.operations(0)
    Wi = np.stack([V.inverse(w) for w in W]).astype(np.float64)
    worst = 0.0
    for k in range(len(W)):
        for l in range(len(W)):
            tt = t2[l] @ Wi[k] + t2[k]
            m = [j for j in range(len(W)) if np.array_equal(Wi[j], Wi[l] @ Wi[k])]
            worst = max(worst, min(float(np.abs((tt - t2[j]) - np.round(tt - t2[j])).max()) for j in m))
    assert worst < 1e-14
    a, x, l = V.random_state(rng, [6])
    assert V.coordinate_defect(c, 0, V.project(c, a, x, l)[1]) <= 1.0


# ---- the kernel's order on the host, under the sanitizers ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("symc") / "sym_constraint_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "sym_constraint_host_check.cpp"), "-o", exe], check=True)
    return exe


def device_arrays(c):
    """The constraint as the kernel reads it: K [B], roff [B + 1], the distinct rotation parts gathered, rep, node_off, Q, d."""
    a = c.arrays()
    B = len(c)
    rot = [a["rot"][a["op_off"][b]:a["op_off"][b + 1]][a["distinct"][a["distinct_off"][b]:a["distinct_off"][b + 1]]] for b in range(B)]
    node_off = np.concatenate([[0], np.cumsum([int(v) for v in c.num_atoms])]).astype(np.int32)
    return dict(K=np.diff(a["op_off"]).astype(np.int32), roff=a["distinct_off"], rot=np.concatenate(rot).astype(np.int32), rep=a["rep"], node_off=node_off,
                Q=a["Q"], d=a["d"])


def run_host_check(exe, tmp_path, c, a, x, l):
    d = device_arrays(c)
    B, N = len(c), c.num_nodes
    cf, of = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(cf, "wb") as f:
        f.write(struct.pack("<iii", B, N, len(d["rot"])))
        for arr, dt in ((d["K"], np.int32), (d["roff"], np.int32), (d["rot"], np.int32), (d["rep"], np.int32), (d["node_off"], np.int32), (d["Q"], np.float64),
                        (d["d"], np.float64), (a, np.float32), (x, np.float32), (l, np.float32)):
            f.write(np.ascontiguousarray(np.asarray(arr, dt)).tobytes())
    r = subprocess.run([exe, cf, of], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(of, "rb").read()
    out, pos = [], 0
    for shape, dt in (((N, 100), np.float32), ((N, 3), np.float32), ((B, 9), np.float32), ((B,), np.int32)):
        size = int(np.prod(shape)) * np.dtype(dt).itemsize
        out.append(np.frombuffer(raw[pos:pos + size], dt).reshape(shape))
        pos += size
    assert pos == len(raw)
    return out


def test_host_check_equals_the_restatement(host_check, tmp_path):
    c = SC.stack([CS.constraint(n) for n in CS.NAMES])
    a, x, l = V.random_state(np.random.default_rng(2024), [int(v) for v in c.num_atoms])
    got = run_host_check(host_check, tmp_path, c, a, x, l)
    for g, r in zip(got, V.project(c, a, x, l)):
        assert g.shape == r.shape and np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, r.view(np.uint32) if r.dtype == np.float32 else r)


def test_host_check_equals_the_restatement_on_the_guards(host_check, tmp_path):
    c, a, x, l = CS.guard_case()
    ref = V.project(c, a, x, l)
    assert ref[3].tolist() == [0, 1, 1, 0, 0]
    assert np.array_equal(bits(ref[2][[1, 2, 3]]), bits(l[[1, 2, 3]])) and not np.array_equal(bits(ref[2][0]), bits(l[0]))
    got = run_host_check(host_check, tmp_path, c, a, x, l)
    for g, r in zip(got, ref):
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, r.view(np.uint32) if r.dtype == np.float32 else r)


def test_header_table_constants_and_the_unit():
    from matinvent_amd.build import ALL_SOURCES, MORE_SOURCES, SOURCES
    names = sorted(declared_symbols("matinvent_hip_symc.h"))
    assert names == ["mi_batch_set_symmetry", "mi_symmetry_apply", "mi_symmetry_failures"] and sorted(_lib.SYMC_SIGNATURES) == names
    assert any(t is _lib.SYMC_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    assert "sym_constraint.hip" in MORE_SOURCES and "sym_constraint.hip" in ALL_SOURCES and len(SOURCES) == 31 and len(set(ALL_SOURCES)) == len(ALL_SOURCES)
    head = open(os.path.join(ROOT, "include", "matinvent_hip_symc.h")).read()
    ops = open(os.path.join(ROOT, "matinvent_amd", "csrc", "sym_constraint.h")).read()
    unit = open(os.path.join(ROOT, "matinvent_amd", "csrc", "sym_constraint.hip")).read()
    assert "#define MI_SYMC_MAX_ATOMS 256\n" in head and "#define MI_SYMC_MAX_OPS 192\n" in head and "SYMC_MAX_ATOMS = 256" in ops
    assert (_lib.SYMC_MAX_ATOMS, _lib.SYMC_MAX_OPS) == (SC.MAX_ATOMS, SC.MAX_OPS) == (V.MAX_ATOMS, V.MAX_OPS) == (256, 192)
    assert '#include "sym_refine.h"' in ops and "fp contract(off)" in ops and '#include "sym_constraint.h"' in unit and "__launch_bounds__(SYMC_THREADS)" in unit
    for word in ("atomic", "mfma", "asm", "pow(", "cbrt", "exp(", "log(", "sin(", "cos(", "fma("):   # + - x /, sqrt and floor only; plain C++
        assert word not in ops, word
    for word in ("atomic", "mfma", "asm"):
        assert word not in unit.split("namespace mi {", 1)[1], word
    fields = [f[0] for f in _lib.SymmetryConstraint._fields_]
    assert fields == ["op_off_host", "rot_host", "distinct_off_host", "distinct_host", "rep_host", "Q_host", "d_host"]
    order = [head.index(" " + f + ";") for f in fields]   # the struct's members in the table's order
    assert order == sorted(order)
    text = open(os.path.join(ROOT, "dropin", "configs", "symmetry", "template.yaml")).read()
    assert "symmetry_template: null" in text and "symmetry_fix_types: false" in text
    # the entries bind and the host-only refusals answer without a GPU
    lib = _lib.load()
    assert lib.mi_batch_set_symmetry(None, None) == _lib.MI_EINVAL and lib.mi_symmetry_apply(None, None, None, None, None) == _lib.MI_EINVAL
    assert lib.mi_symmetry_failures(None, None) == _lib.MI_EINVAL


# ---- the keyword refusals, before any device work ---------------------------------------------------------------------------------------------
def _module(T=20):
    from matinvent_amd.diffcsp import DiffCSPModule
    return DiffCSPModule(decoder=dict(hidden_dim=64, num_layers=2, num_freqs=8, ln=True, edge_style="fc"),
                         beta_scheduler=dict(timesteps=T, scheduler_mode="cosine"),
                         sigma_scheduler=dict(timesteps=T, sigma_begin=0.005, sigma_end=0.5, sigmas_norm=torch.linspace(0.7, 1.3, T + 1)),
                         device="cpu")


def test_sample_refuses_by_name_before_any_device_work(tmp_path):
    from matinvent_amd import pipeline, sampling
    from matinvent_amd.conditioning import Condition
    from matinvent_amd.suite import DiffCSPSuite
    m = _module(20)
    c = SC.stack([CS.constraint("rutile")] * 2)
    for kw, match in ((dict(record=True), "record"), (dict(noise={}), "noise"), (dict(likelihood="free"), "likelihood"), (dict(resample=(2, 3)), "resample"),
                      (dict(guidance=object()), "guidance"), (dict(steer=object()), "steer"), (dict(classifier=object()), "classifier")):
        with pytest.raises(ValueError, match="symmetry together with .*" + match):
            m.sample(c, symmetry=c, **kw)
    with pytest.raises(ValueError, match="symmetry together with .*" + "record"):
        m.respaced(5).sample(c, symmetry=c, record=True)
    csp = _module(20)
    csp.keep_coords = True
    with pytest.raises(ValueError, match="CSP mode"):
        csp.sample(c, symmetry=c)
    with pytest.raises(ValueError, match="atom counts"):
        m.sample(SimpleNamespace(num_atoms=torch.tensor([6, 5])), symmetry=c)
    z = list(CS.crystal("rutile")[1]) * 2
    with pytest.raises(ValueError, match="coordinate or a lattice"):
        m.sample(c, symmetry=c, condition=Condition([6, 6], atom_types=z, known_types=[True] * 12, lattices=np.tile(np.eye(3), (2, 1, 1)), known_lattice=[True, False]))
    with pytest.raises(ValueError, match="orbit"):
        m.sample(c, symmetry=c, condition=Condition([6, 6], atom_types=z[:3] + [9] + z[4:], known_types=[True] * 12))
    # the trajectory layer and the policy-gradient loop
    with pytest.raises(ValueError, match="symmetry"):
        sampling.sample_mdp(2, None, symmetry=c)
    with pytest.raises(ValueError, match="symmetry"):
        sampling.sample_rollout(2, None, symmetry=c)
    suite = DiffCSPSuite("diffcsp", {"batch_size": 4, "num_batches": 1}, {}, device="cpu")
    with pytest.raises(ValueError, match="sample_cfg.symmetry_template"):
        pipeline.MatInventPG(rl_epoch=1, model_suite=suite, reward=None, sample_cfg={"symmetry_template": "/x.json"}, finetune_cfg={},
                             save_dir=str(tmp_path), save_freq=1, device="cpu")
    g = sampling.DiffCSPSampler(batch_size=2, num_batches=1)
    for kw, match in ((dict(condition=Condition.composition([{"Na": 1, "Cl": 1}], 2)), "condition"), (dict(properties_to_condition_on={"gap": 1.0}), "properties_to_condition_on"),
                      (dict(steer=object()), "steer"), (dict(classifier=object()), "classifier")):
        with pytest.raises(ValueError):
            g.generate(m, symmetry_template=SimpleNamespace(), **kw)
    with pytest.raises(ValueError, match="symmetry_fix_types needs symmetry_template"):
        g.generate(m, symmetry_fix_types=True)
    # the pipelines' sample_cfg carries the keys to the sampler
    rl = pipeline.ReinL(rl_epoch=1, model_suite=suite, reward=None, sample_cfg={"symmetry_template": "/x.json", "symmetry_fix_types": True}, finetune_cfg={},
                        save_dir=str(tmp_path), save_freq=1, device="cpu")
    assert rl.sample_cfg.symmetry_template == "/x.json" and rl.sample_cfg.symmetry_fix_types is True


def test_load_template(tmp_path):
    import json
    p = tmp_path / "rutile.json"
    L, z, f = CS.crystal("rutile")
    p.write_text(json.dumps({"lengths": [4.6, 4.6, 2.96], "angles": [90, 90, 90], "species": [int(v) for v in z], "frac_coords": np.asarray(f).tolist()}))
    rec = SC.load_template(str(p))
    assert rec.species == [int(v) for v in z] and rec.frac_coords.shape == (6, 3) and rec.lengths == [4.6, 4.6, 2.96]
    p.write_text(json.dumps({"lengths": [1, 1, 1]}))
    with pytest.raises(ValueError, match="missing"):
        SC.load_template(str(p))
