"""Time composition validity (mi_chem_validity) beside the two host restatements that give the same answers, in one process:

    python scripts/chem_validity_timing.py [--out profiles/chem_validity_timing.json] [--reps 30]

Batches: (a) 256 crystals of 20 atoms with 2 .. 5 elements of the test table (tests/chem_cases.py: test data, not SMACT's); (b) 256 crystals,
each at N = 10^7 combinations exactly (seven lists of ten); (c) one crystal at 10^7 among 255 of the small ones.  Per batch: the three
launches alone (device events around the enqueue, arrays resident); the whole `chemistry.validity` (upload + call + the one read-back, host
clock around a synchronise); the numpy restatement and the itertools restatement of tests/chem_ref.py -- on the whole batch for (a); for
(b) and (c) the numpy form on ONE 10^7 crystal and the itertools form on the first 10^6 combinations of one, each scaled to the batch
(the sample is stated in the row).  Warm-up, then medians over `reps` calls with the spread (min .. max); the kernel's answers are
compared with the restatement's before anything is timed."""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from matinvent_amd import chemistry as CH  # noqa: E402
from tests import chem_cases as CS  # noqa: E402
from tests import chem_ref as R  # noqa: E402


def spread(ts):
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts)}


def time_events(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return spread(ts)


def time_host(fn, reps, warm=1, sync=True):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return spread(ts)


def small_crystals(n, seed=0):
    """n crystals of 20 atoms over 2 .. 5 elements of the test table that have oxidation states."""
    rng = np.random.default_rng(seed)
    zs = [R.Z_OF[s] for s, row in CS.TEST_TABLE.items() if row["ox"]]
    out = []
    for _ in range(n):
        elems = rng.choice(zs, size=int(rng.integers(2, 6)), replace=False)
        types = list(elems) + list(rng.choice(elems, size=20 - len(elems)))
        out.append([int(z) for z in rng.permutation(types)])
    return out


def itertools_sample(lists, counts, ranks, limit):
    """The itertools restatement's loop over the first `limit` combinations."""
    n = 0
    for combo in itertools.islice(itertools.product(*lists), limit):
        if sum(o * c for o, c in zip(combo, counts)) == 0 and R.passes(combo, ranks):
            n += 1
    return n


class Rec:
    def __init__(self, species):
        self.species = species


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chem_validity_timing.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "chem_validity_timing.py measures on the GPU"
    # one table for all three batches: the test table's elements, and the seven-of-ten family on elements the test table lacks
    big = {R.SYMBOLS[40 + e]: row for e, row in enumerate(CS.ten_million().values())}
    table_dict = dict(CS.TEST_TABLE, **big)
    table = CH.ElementTable(table_dict)
    large = list(range(40, 47))
    small = small_crystals(256)
    batches = (("a: 256 crystals of 20 atoms, 2-5 elements of the test table", small),
               ("b: 256 crystals at N = 10^7 each", [large] * 256),
               ("c: one crystal at N = 10^7 among 255 small ones", small[:100] + [large] + small[100:255]))
    rows_z, rank = R.by_z(table_dict)
    t = time.perf_counter()
    ref_large = R.one(large, table_dict, method="numpy")
    numpy_large_s = time.perf_counter() - t
    lists, ranks = [rows_z[z][0] for z in large], [rank[z] for z in large]
    t = time.perf_counter()
    itertools_sample(lists, [1] * 7, ranks, 10 ** 6)
    itertools_1e6_s = time.perf_counter() - t
    results = []
    for name, crystals in batches:
        want = R.batch(crystals, table_dict, table_key="timing")
        recs = [Rec(c) for c in crystals]
        call = CH.ValidityCall(recs, table, device="cuda")
        got = call.launch().read()
        assert all(np.array_equal(getattr(got, k), want[k]) for k in R.KEYS), name
        n_large = sum(1 for c in crystals if c == large)
        row = {"case": name, "crystals": len(crystals), "combinations_total": int(want["n_combos"].sum()), "work_items": int((-(-want["n_combos"] // R.CHUNK)).sum()),
               "valid": int(want["valid"].sum()), "kernel": time_events(call.launch, args.reps),
               "kernel_end_to_end": time_host(lambda: CH.validity(recs, table, device="cuda"), args.reps)}
        if n_large == 0:
            row["numpy_restatement"] = time_host(lambda: [R.one(c, table_dict, method="numpy") for c in crystals], args.host_reps, sync=False)
            row["itertools_restatement"] = time_host(lambda: [R.one(c, table_dict, method="itertools") for c in crystals], args.host_reps, sync=False)
        else:
            row["numpy_restatement"] = {"sample": "one 10^7 crystal, measured once, times the number of such crystals (the small ones left out)",
                                        "one_crystal_ms": 1e3 * numpy_large_s, "scaled_ms": 1e3 * numpy_large_s * n_large}
            row["itertools_restatement"] = {"sample": "the first 10^6 combinations of one 10^7 crystal, measured once, times 10 times the number of such crystals",
                                            "sample_ms": 1e3 * itertools_1e6_s, "scaled_ms": 1e3 * itertools_1e6_s * 10 * n_large}
        results.append(row)
        print(json.dumps(row), flush=True)
    assert ref_large["n_combos"] == 10 ** 7
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "one_workgroup_per_crystal_form": "not built, not measured", "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
