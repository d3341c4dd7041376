"""GPU checks of the symmetry constraint's kernel (matinvent_amd/csrc/sym_constraint.hip, include/matinvent_hip_symc.h):
mi_symmetry_apply equals the float64 restatement tests/symc_ref64.py BIT FOR BIT -- coordinates, cells, type rows and failure counts,
every crystal, no tolerance -- on the cases of tests/symc_cases.py, a grid of 300 crystals and the guard batch; what
mi_batch_set_symmetry refuses leaves the handle as it was; and the symmetry finder reads the full group off a projected state."""
import ctypes as C

import numpy as np
import pytest
import torch

import tests.test_gpu_respaced_chain as RC
from matinvent_amd import _lib
from matinvent_amd import symmetry_constraint as SC
from tests import symc_cases as CS
from tests import symc_ref64 as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def base():
    return RC._base()[0]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def apply_on_device(base, c, a, x, l, times=1):
    """The state after `times` applications on a fresh handle, and the failure counts."""
    cb = base.make_batch([int(v) for v in c.num_atoms])
    c.attach(cb)
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda().contiguous() for v in (a, x, l.reshape(-1, 3, 3))]
    for _ in range(times):
        SC.apply(cb, *dev)
    fail = SC.failures(cb)
    assert SC.failures(cb).tolist() == [0] * len(c)   # read and cleared
    SC.SymmetryConstraint.clear(cb)
    return dev[0].cpu().numpy(), dev[1].cpu().numpy(), dev[2].cpu().numpy().reshape(-1, 9), fail


def assert_equal_bits(got, ref, what):
    for name, g, r in zip(("atom_types", "frac", "lattices"), got[:3], ref[:3]):
        assert g.shape == r.shape and g.dtype == r.dtype == np.float32, (what, name)
        bad = np.where(bits(g) != bits(r))
        assert len(bad[0]) == 0, (what, name, len(bad[0]), [int(v[0]) for v in bad])
    assert got[3].tolist() == ref[3].tolist(), (what, "failures")


@pytest.mark.parametrize("name", CS.NAMES + ("all",))
def test_apply_equals_the_restatement_bit_for_bit(base, name):
    c = SC.stack([CS.constraint(n) for n in CS.NAMES]) if name == "all" else CS.constraint(name)
    na = [int(v) for v in c.num_atoms]
    a, x, l = V.random_state(np.random.default_rng(5600 + len(na) + sum(na)), na)
    ref = V.project(c, a, x, l)
    got = apply_on_device(base, c, a, x, l)
    assert_equal_bits(got, ref, name)
    for i in range(len(c)):
        lo, hi = sum(na[:i]), sum(na[:i + 1])
        assert V.coordinate_defect(c, i, got[1][lo:hi]) <= 1.0 and V.orbits_share_rows(c, i, got[0][lo:hi])
        assert got[3][i] != 0 or V.cell_defect(c, i, got[2][i]) <= 1.0
    # a second application on the device is the restatement's second application
    assert_equal_bits(apply_on_device(base, c, a, x, l, times=2)[:3] + (ref[3],), V.project(c, *ref[:3])[:3] + (ref[3],), name + " twice")


def test_a_grid_of_300_crystals(base):
    c = CS.batch_300()
    na = [int(v) for v in c.num_atoms]
    assert len(na) == 300 and max(na) == 8 and c.num_ops[0] == c.num_ops[150] == c.num_ops[299] == 192
    a, x, l = V.random_state(np.random.default_rng(300), na)
    assert_equal_bits(apply_on_device(base, c, a, x, l), V.project(c, a, x, l), "grid")


def test_the_guard_batch(base):
    c, a, x, l = CS.guard_case()
    ref = V.project(c, a, x, l)
    got = apply_on_device(base, c, a, x, l)
    assert_equal_bits(got, ref, "guards")
    assert got[3].tolist() == CS.GUARD_FAILURES
    assert np.array_equal(bits(got[2][[1, 2, 3]]), bits(l[[1, 2, 3]]))          # the failed cells and the free crystal's: every bit kept
    na = [int(v) for v in c.num_atoms]
    free = slice(sum(na[:3]), sum(na[:4]))
    assert np.array_equal(bits(got[0][free]), bits(a[free])) and np.array_equal(bits(got[1][free]), bits(x[free]))
    # the coordinates and type rows of a crystal whose cell failed are projected all the same
    assert V.coordinate_defect(c, 1, got[1][6:12]) <= 1.0 and V.orbits_share_rows(c, 2, got[0][12:18])
    # the counters add up over applications until they are read
    cb = base.make_batch(na)
    c.attach(cb)
    dev = [torch.from_numpy(v).cuda().contiguous() for v in (a, x, l.reshape(-1, 3, 3))]
    SC.apply(cb, *dev)
    SC.apply(cb, *dev)
    assert SC.failures(cb).tolist() == [0, 2, 2, 0, 0]
    SC.SymmetryConstraint.clear(cb)


def _set(cb, arrays):
    keep = [np.ascontiguousarray(arrays[k]) for k in ("op_off", "rot", "distinct_off", "distinct", "rep", "Q", "d")]
    st = _lib.SymmetryConstraint(*(v.ctypes.data for v in keep))
    return _lib.load().mi_batch_set_symmetry(cb._h, C.byref(st))


def test_set_symmetry_refusals_leave_the_handle_usable(base):
    c = SC.stack([CS.constraint("rutile"), CS.constraint("p1bar_pair")])
    na = [6, 2]
    a, x, l = V.random_state(np.random.default_rng(77), na)
    ref = V.project(c, a, x, l)
    cb = base.make_batch(na)
    c.attach(cb)
    good = c.arrays()

    def changed(**kw):
        arr = {k: np.array(v, copy=True) for k, v in good.items()}
        for k, (idx, val) in kw.items():
            arr[k][idx] = val
        return arr

    wide = {k: np.array(v, copy=True) for k, v in good.items()}            # 193 operations: K outside 1..192
    wide["op_off"] = np.array([0, 193, 195], np.int32)
    wide["rot"] = np.concatenate([np.tile(good["rot"][:1], (193, 1)), good["rot"][16:]])
    empty = {k: np.array(v, copy=True) for k, v in good.items()}           # no operation at all
    empty["op_off"] = np.array([0, 0, 2], np.int32)
    cases = {"a representative outside its crystal": changed(rep=(7, 2)), "a negative representative": changed(rep=(0, -1)),
             "not its own representative": changed(rep=(3, 4)), "K = 193": wide, "K = 0": empty, "a non-finite Q": changed(Q=((2, 4), np.nan)),
             "a non-finite d": changed(d=((7, 0), np.inf)), "det W = 2": changed(rot=(3, [2, 0, 0, 0, 1, 0, 0, 0, 1])),
             "a distinct entry outside": changed(distinct=(1, 16)), "a distinct entry twice": changed(distinct=(1, 0))}
    for what, arr in cases.items():
        assert _set(cb, arr) == _lib.MI_EINVAL, what
        dev = [torch.from_numpy(v).cuda().contiguous() for v in (a, x, l.reshape(-1, 3, 3))]
        SC.apply(cb, *dev)                                                  # the handle still carries the good constraint
        got = (dev[0].cpu().numpy(), dev[1].cpu().numpy(), dev[2].cpu().numpy().reshape(-1, 9), SC.failures(cb))
        assert_equal_bits(got, ref, what)
    # more than 256 atoms under more than the identity
    big = base.make_batch([257])
    two = dict(op_off=np.array([0, 2], np.int32), rot=np.stack([np.eye(3), -np.eye(3)]).reshape(2, 9).astype(np.int32), distinct_off=np.array([0, 2], np.int32),
               distinct=np.array([0, 1], np.int32), rep=np.arange(257, dtype=np.int32), Q=np.tile(np.eye(3).reshape(1, 9), (257, 1)), d=np.zeros((257, 3)))
    assert _set(big, two) == _lib.MI_EINVAL
    with pytest.raises(_lib.MIError) as e:                                  # ... and no constraint came to be attached
        SC.apply(big, torch.zeros(257, 100, device="cuda"), torch.zeros(257, 3, device="cuda"), torch.zeros(1, 3, 3, device="cuda"))
    assert e.value.code == _lib.MI_EINVAL
    SC.SymmetryConstraint.identity([257]).attach(big)                       # the identity has no atom cap
    SC.SymmetryConstraint.clear(big)
    SC.SymmetryConstraint.clear(cb)
    with pytest.raises(ValueError, match="atom counts"):
        c.attach(base.make_batch([6, 3]))


def test_the_finder_reads_192_operations_off_a_projected_state(base):
    """Random coordinates and a healthy cell (5.6 A cubic, every entry disturbed by up to 0.4 A) projected onto conventional rock salt: the
    finder at symprec = 1e-3 reports all 192 operations."""
    from matinvent_amd.data import SimpleStructure
    from matinvent_amd.symmetry import find_symmetry
    from tests import refine_ref64 as RR
    c = CS.constraint("rocksalt_conv")
    rng = np.random.default_rng(192)
    a, x, _ = V.random_state(rng, [8])
    a[0, 10], a[4, 16] = 9.0, 9.0                                            # the two orbits are two species: Na, Cl
    l = (np.eye(3) * 5.6 + rng.uniform(-0.4, 0.4, (3, 3))).astype(np.float32).reshape(1, 9)
    ta, tx, tl, fail = apply_on_device(base, c, a, x, l)
    assert fail.tolist() == [0]
    species = [int(v) + 1 for v in ta.argmax(1)]
    assert species == [11] * 4 + [17] * 4
    p = RR.cell_parameters(tl[0].astype(np.float64).reshape(3, 3))
    res = find_symmetry([SimpleStructure(p[:3], p[3:], species, tx.astype(np.float64))], symprec=1e-3)
    assert int(res.status[0]) == _lib.SYM_OK and int(res.n_ops[0]) == 192 and res.point_group[0] == "m-3m"
