"""CPU checks of the long-term memory and the structure-keyed memories (matinvent_amd/memory.py): LongTimeMem against the call
sequence the reference's own class produced (tests/golden/g14_ltm.json, written by tests/golden/make_golden_ltm.py), rewards compared
exactly; ReplayBuffer's composition key unchanged; and the structure-key logic with fingerprints injected as arrays -- no device."""
import csv
import json
import math
import os

import numpy as np
import pytest

from matinvent_amd.data import SimpleStructure
from matinvent_amd.memory import LongTimeMem, ReplayBuffer
from matinvent_amd.structure import SYMBOLS, reduced_formula

HERE = os.path.dirname(os.path.abspath(__file__))


def _struc(symbols):
    n = len(symbols)
    return SimpleStructure([4.0, 5.0, 6.0], [90.0, 90.0, 90.0], [SYMBOLS.index(s) for s in symbols], np.linspace(0, 0.9, 3 * n).reshape(n, 3))


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and ((math.isnan(a) and math.isnan(b)) or a == b))


def test_long_time_mem_reproduces_the_reference_call_for_call(tmp_path):
    calls = json.load(open(os.path.join(HERE, "golden", "g14_ltm.json")))["calls"]
    ops = [c["op"] for c in calls]
    assert ops.count("div_filter") >= 8 and ops.count("extend") >= 6
    assert any(c["op"] == "calc_metrics" and c["burden"] is not None for c in calls) and any(c["op"] == "calc_metrics" and c["burden"] is None for c in calls)
    assert any(c["op"] == "calc_metrics" and c["div_ratio"] is None for c in calls)
    assert {c["kw"].get("method", "composition") for c in calls if c["op"] == "div_filter"} == {"composition", "element_comb"}
    mem = LongTimeMem()
    scaled = zeroed = 0
    for c in calls:
        if c["op"] == "extend":
            mem.extend([_struc(s) for s in c["species"]], np.array(c["rewards"]), c["step"])
            assert list(mem.unique_comps) == c["unique_comps"] and len(mem) == c["length"]
        elif c["op"] == "calc_metrics":
            burden, div_ratio = mem.calc_metrics(c["thred"], **c["kw"])
            assert _same(burden, c["burden"]) and _same(div_ratio, c["div_ratio"]), c
        elif c["op"] == "get_baseline":
            b = mem.get_baseline(c["step"], **c["kw"])
            assert _same(None if math.isnan(b) else b, c["baseline"]), c
        else:
            new, pen, tol_n, buff_n = mem.div_filter([_struc(s) for s in c["species"]], np.array(c["rewards"]), **c["kw"])
            assert new.tolist() == c["new_rewards"], c                      # the same float64 operations: exact
            assert (list(pen), tol_n, buff_n) == (c["penalty_idx"], c["tol_n"], c["buff_n"]), c
            scaled, zeroed = scaled + tol_n, zeroed + buff_n
    assert scaled > 0 and zeroed > 0
    with pytest.raises(AssertionError):
        mem.div_filter([], np.zeros(0), tol=5, buff=5)
    path = tmp_path / "long_term_memory.csv"
    mem.save(str(path))
    rows = list(csv.reader(open(path, newline="")))
    assert rows[0] == ["struc", "comp", "ele_comb", "reward", "RL_step", "cif"] and len(rows) == len(mem) + 1
    assert rows[1][1] == "Li2O" and rows[1][5].startswith("data_generated") and "_cell_length_a   4.000000" in rows[1][5]
    assert open(path).read().startswith('"struc","comp"')               # every field quoted


class _Data:
    """What the replay buffer stores: a record with atom_types."""

    def __init__(self, species, tag):
        self.atom_types, self.tag = np.array(species), tag


def test_replay_buffer_composition_key_is_unchanged():
    g = np.random.default_rng(0)
    pool = [[3, 3, 8], [11, 17], [3, 8], [3, 3, 3, 3, 8, 8], [26, 8]]
    buf = ReplayBuffer(buffer_size=3, sample_size=2, reward_cutoff=0.1, seed=4)
    assert buf.key == "composition"
    best = {}
    for step in range(4):
        data = [_Data(pool[int(k)], (step, i)) for i, k in enumerate(g.integers(0, len(pool), 5))]
        rewards = g.random(5)
        buf.extend(data, None, rewards)
        for d, r in zip(data, rewards):
            f = reduced_formula(d.atom_types.tolist())
            best[f] = max(best.get(f, 0.0), float(r))
        want = sorted((r for r in best.values()), reverse=True)[:3]
        assert [row[0] for row in buf.rows] == [r for r in want if r > 0.1] and all(len(row) == 3 for row in buf.rows)
    assert len({row[1] for row in buf.rows}) == len(buf.rows)
    d, r = buf.sample()
    assert len(d) == 2 and len(r) == 2
    buf.memory_purge([_struc(["Li", "Li", "O"])])
    assert "Li2O" not in {row[1] for row in buf.rows}
    with pytest.raises(ValueError):
        ReplayBuffer(key="symmetry")


# ---- the structure key, fingerprints injected -----------------------------------------------------------------------------------------

def _unit(angle_deg):
    """Unit vectors in a plane: the cosine distance of two of them is (1 - cos(difference)) / 2."""
    a = math.radians(angle_deg)
    return np.array([math.cos(a), math.sin(a), 0.0], np.float32)


TOL = 0.5 * (1 - math.cos(math.radians(10.0)))     # two vectors are one structure up to 10 degrees apart
LI2O = ["Li", "Li", "O"]


def _fps(angles, flagged=()):
    return np.stack([_unit(a) for a in angles]), np.array([4 if i in flagged else 0 for i in range(len(angles))])


def test_leader_clustering_is_in_insertion_order():
    mem = LongTimeMem(structure=True, fp_tol=TOL)
    s = [_struc(LI2O) for _ in range(5)]
    # 0 founds A; 8 joins A; 16 is 8 from the second row but 16 from A's founder: founds B; 12 joins A?  no -- 12 > 10 from 0, 4 from 16: B
    mem.extend(s[:4], np.ones(4), 0, fingerprints=_fps([0, 8, 16, 12]))
    assert [r["cluster"] for r in mem.memory] == [("Li2O", 0), ("Li2O", 0), ("Li2O", 1), ("Li2O", 1)]
    assert mem.unique_structures == 2 and list(mem.unique_comps) == ["Li2O"]
    # the other order founds other clusters: 16 first, then 8 (joins), 0 (founds), 12 (joins the FIRST within reach: 16's)
    other = LongTimeMem(structure=True, fp_tol=TOL)
    other.extend(s[:4], np.ones(4), 0, fingerprints=_fps([16, 8, 0, 12]))
    assert [r["cluster"][1] for r in other.memory] == [0, 0, 1, 0]
    # another formula never shares a cluster, whatever its fingerprint
    mem.extend([_struc(["Na", "Cl"])], np.ones(1), 1, fingerprints=_fps([0]))
    assert mem.memory[-1]["cluster"] == ("ClNa", 0) and mem.unique_structures == 3
    # occ is the cluster's count, the batch's own members included; composition would have counted 4 for every row
    new, pen, tol_n, buff_n = mem.div_filter(s[:4], np.array([1.0, 1.0, 1.0, 1.0]), tol=1, buff=3, method="structure", fp_tol=TOL)
    assert new.tolist() == [0.5, 0.5, 0.5, 0.5] and pen == [] and (tol_n, buff_n) == (4, 0)
    comp, pen_c, _, _ = mem.div_filter(s[:4], np.ones(4), tol=1, buff=3)
    assert comp.tolist() == [0.0] * 4 and pen_c == [0, 1, 2, 3]
    # a crystal that was never stored is looked up, not added
    new, pen, _, _ = mem.div_filter([s[4]], np.ones(1), tol=1, buff=2, method="structure", fingerprints=_fps([40]))
    assert new.tolist() == [1.0] and mem.unique_structures == 3
    new, pen, _, _ = mem.div_filter([s[4]], np.ones(1), tol=1, buff=2, method="structure", fingerprints=_fps([3]))
    assert new.tolist() == [0.0] and pen == [0]
    with pytest.raises(ValueError):
        LongTimeMem().div_filter(s[:1], np.ones(1), method="structure")
    with pytest.raises(ValueError):
        mem.div_filter(s[:1], np.ones(1), method="structure", fp_tol=2 * TOL)


def test_flagged_crystals_are_keyed_by_formula_alone():
    mem = LongTimeMem(structure=True, fp_tol=TOL)
    s = [_struc(LI2O) for _ in range(4)]
    mem.extend(s, np.ones(4), 0, fingerprints=_fps([0, 0, 0, 0], flagged=(1, 3)))   # flagged rows are zero rows in practice; the status decides
    assert [r["cluster"] for r in mem.memory] == [("Li2O", 0), ("Li2O", -1), ("Li2O", 0), ("Li2O", -1)]
    assert len(mem._reps["Li2O"]) == 1 and mem.unique_structures == 2            # one fingerprint per cluster is stored, none for the flagged
    new, pen, _, _ = mem.div_filter(s, np.ones(4), tol=1, buff=3, method="structure")
    assert new.tolist() == [0.5] * 4


def test_structure_keyed_replay_keeps_distinct_structures_of_one_formula():
    data = [_Data([3, 3, 8], i) for i in range(8)]
    rewards = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2])
    angles = [0, 30, 60, 90, 120, 150, 5, 35]                                     # the last two repeat the first two structures
    comp = ReplayBuffer(buffer_size=4, sample_size=2)
    comp.extend(data, None, rewards)
    assert len(comp) == 1                                                          # one formula: one row
    buf = ReplayBuffer(buffer_size=4, sample_size=2, key="structure", fp_tol=TOL)
    buf.extend(data, None, rewards, fingerprints=_fps(angles))
    assert len(buf) == 4 and [row[2].tag for row in buf.rows] == [0, 1, 2, 3]
    # a better copy of a stored structure replaces it; a worse one is dropped
    buf.extend([_Data([3, 3, 8], 8), _Data([3, 3, 8], 9)], None, np.array([0.95, 0.1]), fingerprints=_fps([62, 91]))
    assert [row[2].tag for row in buf.rows] == [8, 0, 1, 3] and [row[0] for row in buf.rows] == [0.95, 0.9, 0.8, 0.6]
    # flagged rows: by formula alone, among themselves
    buf.extend([_Data([3, 3, 8], 10), _Data([3, 3, 8], 11)], None, np.array([0.99, 0.98]), fingerprints=_fps([0, 0], flagged=(0, 1)))
    assert [row[2].tag for row in buf.rows] == [10, 8, 0, 1] and buf.rows[0][3] is None
    # purge by structure: the structure at 30 degrees and the flagged key go, the others stay
    buf.memory_purge([_struc(LI2O), _struc(LI2O)], fingerprints=_fps([28, 0], flagged=(1,)))
    assert [row[2].tag for row in buf.rows] == [8, 0]
    buf.memory_purge([_struc(["Na", "Cl"])], fingerprints=_fps([0]))              # another formula: nothing
    assert len(buf) == 2
