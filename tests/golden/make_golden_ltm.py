#!/usr/bin/env python
"""Generate g14_ltm.json by running the reference's own LongTimeMem (memory/ltm.py) on a recorded call sequence.

Like make_golden.py, this runs only where the reference checkout exists (its directory is taken from the environment variable
MATINVENT_REFERENCE); the tests read the committed json alone.  The reference module is imported through tests/oracle_shims (pymatgen
and torch_geometric are only named in its annotations); the structures are duck-typed here: `.species` (element symbols) and
`.composition.reduced_formula` (this project's spelling, matinvent_amd.structure.reduced_formula: the key only has to be canonical).

g14: data only -- per call its inputs and what the reference returned: after every `extend` the unique compositions, the length, and
calc_metrics / get_baseline; for every `div_filter` the new rewards, the penalised indices and the two counters.  The sequence covers both
methods, occurrences at tol, tol + 1, buff - 1 and buff, a batch whose own members push a key over tol, burden None and not None, and
div_ratio past its budget.
Usage: MATINVENT_REFERENCE=/path/to/reference python tests/golden/make_golden_ltm.py
"""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests", "oracle_shims"))
sys.path.insert(0, ROOT)

from matinvent_amd.structure import SYMBOLS, reduced_formula  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_ltm", os.path.join(os.environ["MATINVENT_REFERENCE"], "memory", "ltm.py"))
ref_ltm = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref_ltm)


class _Comp:
    def __init__(self, formula):
        self.reduced_formula = formula


class Struc:
    def __init__(self, symbols):
        self.species = list(symbols)
        self.composition = _Comp(reduced_formula(SYMBOLS.index(s) for s in symbols))


POOL = [["Li", "Li", "O"], ["Na", "Cl"], ["Li", "O", "O", "Li", "Li", "Li"], ["Li", "O"], ["Si", "O", "O"], ["Fe", "O"], ["Na", "Na", "Cl", "Cl"],
        ["Mg", "O"], ["Ti", "O", "O"], ["Li", "Fe", "O", "O"]]


def jsonable(v):
    if isinstance(v, (np.floating, float)):
        return None if np.isnan(v) else float(v)
    if isinstance(v, (np.integer, int)):
        return int(v)
    if isinstance(v, (list, tuple, np.ndarray)):
        return [jsonable(x) for x in v]
    return v


def main():
    g = np.random.default_rng(14)
    mem = ref_ltm.LongTimeMem()
    calls = []

    def extend(batch, step):
        rewards = g.random(len(batch)).round(6)
        mem.extend([Struc(s) for s in batch], rewards, step)
        calls.append(dict(op="extend", species=batch, rewards=jsonable(rewards), step=step, unique_comps=list(mem.unique_comps), length=len(mem)))

    def metrics(thred, **kw):
        burden, div_ratio = mem.calc_metrics(thred, **kw)
        calls.append(dict(op="calc_metrics", thred=thred, kw=kw, burden=jsonable(burden), div_ratio=jsonable(div_ratio)))

    def baseline(step, **kw):
        calls.append(dict(op="get_baseline", step=step, kw=kw, baseline=jsonable(mem.get_baseline(step, **kw))))

    def filt(batch, **kw):
        rewards = g.random(len(batch)).round(6)
        new, pen, tol_n, buff_n = mem.div_filter([Struc(s) for s in batch], rewards, **kw)
        calls.append(dict(op="div_filter", species=batch, rewards=jsonable(rewards), kw=kw, new_rewards=jsonable(new), penalty_idx=jsonable(pen),
                          tol_n=int(tol_n), buff_n=int(buff_n)))

    baseline(0)                                                            # empty memory: nan
    # step 0: Li2O twice (Li2O and Li4O2), NaCl once; tol 2, buff 5
    extend([POOL[0], POOL[1], POOL[2]], 0)
    metrics(0.5)
    metrics(0.0, num_candidate=2)                                          # burden not None
    filt([POOL[0], POOL[1], POOL[3]], tol=2, buff=5)                       # occ 2 = tol, 1, 0
    filt([POOL[0], POOL[3]], tol=2, buff=5, method="element_comb")         # ("Li", "O"): occ 2 with LiO unseen as a composition
    # step 1: the batch's own members push Li2O over tol (3 = tol + 1) -- the pipeline extends before it filters
    batch = [POOL[0], POOL[4], POOL[5]]
    extend(batch, 1)
    filt(batch, tol=2, buff=5)
    extend([POOL[2]], 1)                                                   # occ 4 = buff - 1
    filt([POOL[0]], tol=2, buff=5)
    extend([POOL[0]], 2)                                                   # occ 5 = buff
    filt([POOL[0], POOL[2], POOL[1]], tol=2, buff=5)
    filt([POOL[0], POOL[9], POOL[5]], tol=2, buff=5, method="element_comb")
    filt([POOL[0], POOL[1]])                                               # the defaults, tol 10 / buff 20
    baseline(2)
    baseline(2, prev=1)
    baseline(9)
    for step in range(3, 6):
        extend([POOL[int(k)] for k in g.integers(0, len(POOL), 6)], step)
        metrics(0.3, num_candidate=3)
        metrics(0.99, num_candidate=3)
    metrics(0.3, budget=len(mem))                                          # cost == budget: a ratio
    metrics(0.3, budget=len(mem) - 1)                                      # past the budget: None
    filt([p for p in POOL], tol=3, buff=6)
    filt([p for p in POOL], tol=3, buff=6, method="element_comb")
    baseline(5)

    path = os.path.join(HERE, "g14_ltm.json")
    with open(path, "w") as f:
        json.dump(dict(calls=calls), f, indent=1)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB, {len(calls)} calls)")


if __name__ == "__main__":
    main()
