"""energy_analysis.py without a device: the pipelined driver's order of calls, its refusal fallback and its clean-up, records -> float32
state, and the configuration the four analyses share."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from matinvent_amd import _lib, energy_analysis as EA


def _driver(groups, batch_size, refuse=(), fail_at=None, max_pending=2):
    """run_pipelined on fakes that log: enqueue raises MIError for a state that holds a row of `refuse`, RuntimeError at its fail_at-th call."""
    log, alive, peak, calls = [], [], [0], [0]

    def enqueue(key, rows):
        calls[0] += 1
        if calls[0] == fail_at:
            raise RuntimeError("enqueue (test)")
        if set(rows) & set(refuse):
            raise _lib.MIError(-5, "refused (test)")
        log.append(("enqueue", key, tuple(rows)))
        alive.append(tuple(rows))
        peak[0] = max(peak[0], len(alive))
        return key, tuple(rows)

    def read(state):
        log.append(("read",) + state)
        alive.remove(state[1])

    def release(state):
        log.append(("release",) + state)
        alive.remove(state[1])

    try:
        ran, err = EA.run_pipelined(groups, batch_size, enqueue, read, release, max_pending=max_pending), None
    except RuntimeError as e:
        ran, err = None, e
    return log, ran, err, peak[0], alive


def test_a_state_is_read_behind_the_next_enqueue():
    log, ran, err, peak, alive = _driver([(None, [0, 1, 2, 3, 4])], 2)
    assert [(k, r) for k, _, r in log] == [("enqueue", (0, 1)), ("enqueue", (2, 3)), ("read", (0, 1)), ("enqueue", (4,)), ("read", (2, 3)), ("read", (4,))]
    assert ran is True and err is None and peak == 2 and alive == []
    assert _driver([(None, [])], 2)[:2] == ([], False)
    # max_pending = None: every read at the end, in the order of the enqueues
    log, ran, _, peak, alive = _driver([(None, [0, 1, 2, 3, 4])], 2, max_pending=None)
    assert [k for k, _, _ in log] == ["enqueue"] * 3 + ["read"] * 3 and [r for _, _, r in log[3:]] == [(0, 1), (2, 3), (4,)] and peak == 3 and alive == []


def test_a_refused_state_runs_row_by_row():
    log, ran, err, peak, alive = _driver([(None, [0, 1, 2, 3, 4])], 2, refuse=(2,))
    assert [(k, r) for k, _, r in log] == [("enqueue", (0, 1)), ("enqueue", (3,)), ("read", (0, 1)), ("enqueue", (4,)), ("read", (3,)), ("read", (4,))]
    assert ran is True and err is None and peak == 2 and alive == []
    assert not any(2 in r for _, _, r in log) and not any(k == "release" for k, _, _ in log)
    # nothing but refusals: nothing ran
    assert _driver([(None, [2])], 2, refuse=(2,))[:2] == ([], False)


def test_another_error_releases_what_is_pending_and_propagates():
    log, ran, err, peak, alive = _driver([(None, [0, 1, 2, 3, 4])], 2, fail_at=2)
    assert isinstance(err, RuntimeError) and [(k, r) for k, _, r in log] == [("enqueue", (0, 1)), ("release", (0, 1))] and alive == []


def test_groups_are_never_mixed_in_one_state():
    log, ran, _, peak, alive = _driver([("a", [0, 1, 2]), ("b", [3, 4])], 2)
    assert [(k, g, r) for k, g, r in log if k == "enqueue"] == [("enqueue", "a", (0, 1)), ("enqueue", "a", (2,)), ("enqueue", "b", (3, 4))]
    assert [r for k, _, r in log if k == "read"] == [(0, 1), (2,), (3, 4)] and ran is True and peak == 2 and alive == []


def test_pack_records_is_the_hand_built_state():
    from matinvent_amd.data import SimpleStructure
    from matinvent_amd.predictor import _valid_fields
    from matinvent_amd.structure import MASSES, lattice_matrix
    recs = [SimpleStructure([4.0, 4.5, 5.0], [90.0, 90.0, 90.0], [14], np.array([[-0.25, 0.5, 1.0]])),
            SimpleStructure([4.0, 4.0, 6.0], [90.0, 90.0, 120.0], [3, 8], np.array([[0.1, 0.2, 0.3], [1.0, -0.25, 0.7]])),
            SimpleStructure([5.0, 5.5, 6.0], [80.0, 95.0, 100.0], [100, 1, 26], np.array([[0.0, 0.0, 0.0], [0.3, 1.25, -1.0e-9], [0.5, 0.5, 0.5]]))]
    fields = [_valid_fields(r) for r in recs]
    na, (frac, lat, types), mass = EA.pack_records(fields, [0, 1, 2], "cpu", masses=True)
    # by hand, as tests/test_gpu_vib_e2e.py's _mixed builds the state of its records
    z = np.array(sum((r.species for r in recs), []))
    t = np.zeros((z.size, 100), np.float32)
    t[np.arange(z.size), z - 1] = 1.0
    x = (np.concatenate([r.frac_coords for r in recs]) % 1.0).astype(np.float32)
    L = np.stack([lattice_matrix(r.lengths, r.angles) for r in recs]).astype(np.float32)
    assert na == [1, 2, 3] and types.dtype == frac.dtype == lat.dtype == torch.float32 and tuple(types.shape) == (6, 100) == (6, _lib.NUM_TYPES)
    assert np.array_equal(types.numpy(), t) and (types.sum(1) == 1).all() and types.numpy().argmax(1).tolist() == (z - 1).tolist()
    assert np.array_equal(frac.numpy().view(np.int32), x.view(np.int32)) and np.array_equal(lat.numpy().view(np.int32), L.view(np.int32))
    assert frac[0].tolist() == [0.75, 0.5, 0.0] and frac[2].tolist() == [0.0, 0.75, np.float32(0.7)]
    assert frac[4, 2] == np.float32(-1.0e-9 % 1.0) == 1.0   # wrapped in float64 first: the float32 of 1 - 1e-9, not a float32 remainder
    assert mass.dtype == np.float64 and np.array_equal(mass, np.asarray(MASSES, dtype=np.float64)[z])
    # a subset in another order, without masses
    na2, (frac2, lat2, types2) = EA.pack_records(fields, [2, 0], "cpu")
    assert na2 == [3, 1] and torch.equal(frac2, torch.cat([frac[3:], frac[:1]])) and torch.equal(lat2, lat[[2, 0]]) and torch.equal(types2, torch.cat([types[3:], types[:1]]))


def _classes():
    from matinvent_amd.elasticity import Elasticity
    from matinvent_amd.phonons import Phonons
    from matinvent_amd.relax import Relaxer
    from matinvent_amd.vibrations import Vibrations
    return Vibrations, Elasticity, Phonons, Relaxer


@pytest.mark.parametrize("k", range(4))
def test_the_four_analyses_share_their_configuration(k):
    cls = _classes()[k]
    who = cls.__name__
    pred = SimpleNamespace(names=["gap", "energy"], hparams={}, normalizer=SimpleNamespace(std=[1.0, 2.5]), P=2, device="cpu")
    a = cls(pred, "energy", batch_size=7, det_min=0.01, per_atom=False)
    assert isinstance(a, EA.EnergyAnalysis) and a.predictor is pred and (a.task, a.p, a.per_atom, a.batch_size, a.det_min) == ("energy", 1, False, 7, 0.01)
    assert a.scale() == 2.5
    import copy
    assert copy.deepcopy(a) is a and copy.deepcopy(dict(x=a))["x"] is a
    with pytest.raises(ValueError, match=f"{who}: a knn-style predictor"):
        cls(SimpleNamespace(names=["energy"], hparams=dict(edge_style="knn")), "energy")
    with pytest.raises(ValueError, match=f"{who}: task = 'volume'"):
        cls(pred, "volume")
    for bad in (0.0, float("nan"), -1.0, float("inf")):
        with pytest.raises(ValueError, match=f"{who}: det_min"):
            cls(pred, "energy", det_min=bad)
    with pytest.raises(ValueError, match=f"{who}: batch_size = 0"):
        cls(pred, "energy", batch_size=0)
    if who == "Relaxer":
        assert not hasattr(a, "delta") and a.fire["det_min"] == 0.01
        with pytest.raises(ValueError, match="Relaxer: unknown keywords"):
            cls(pred, "energy", delta=0.0)
    else:
        assert cls(pred, "energy", delta=0.02).delta == 0.02
        for bad in (0.0, float("nan")):
            with pytest.raises(ValueError, match=f"{who}: delta"):
                cls(pred, "energy", delta=bad)
    for std in (0.0, float("nan")):
        with pytest.raises(ValueError, match=f"{who}: the normaliser's std of 'energy'"):
            cls(SimpleNamespace(names=["energy"], hparams={}, normalizer=SimpleNamespace(std=[std])), "energy").scale()


def test_what_each_analysis_keeps_of_its_own():
    Vibrations, Elasticity, Phonons, Relaxer = _classes()
    pred = SimpleNamespace(names=["energy"], hparams={}, normalizer=SimpleNamespace(std=[1.0]), P=1, device="cpu")
    v, e, p, r = Vibrations(pred, "energy"), Elasticity(pred, "energy"), Phonons(pred, "energy"), Relaxer(pred, "energy")
    assert (v.delta, v.temperatures, v.nu_cut, v.batch_size, v.supercell, v.det_min, v.per_atom) == (0.01, (300.0,), 0.05, 256, (1, 1, 1), 1e-3, True)
    assert (e.delta, e.ion_steps, e.batch_size, e.det_min, e.fire["fmax"]) == (0.005, 0, 256, 1e-3, 0.1)
    assert (p.delta, p.temperatures, p.nu_cut, p.supercell, p.min_length, p.mesh, p.tie_tol, p.batch_size) == (0.01, (300.0,), 0.05, (2, 2, 2), 10.0, (4, 4, 4), 1e-5, 256)
    assert (r.steps, r.check_every, r.batch_size, r.relax_cell, r.per_atom, r.cell_factor, r.last_info) == (50, 0, 64, True, True, None, None)
    assert not isinstance(p, Vibrations)   # (no throw-away Vibrations inside a Phonons either: scale is the class's own method)
    assert p.scale.__func__ is EA.EnergyAnalysis.scale
    assert r.params().scale == 1.0 and r.params().det_min == np.float32(1e-3)
    for cls in (Vibrations, Phonons):   # a Phonons refusal names Phonons
        with pytest.raises(ValueError, match=f"{cls.__name__}: temperatures"):
            cls(pred, "energy", temperatures=())
        with pytest.raises(ValueError, match=f"{cls.__name__}: nu_cut"):
            cls(pred, "energy", nu_cut=-1.0)
    from matinvent_amd import phonons, vibrations
    assert vibrations._at is EA._at and phonons._at is EA._at and vibrations.release_handles is EA.release_handles
