"""Time the energy above the convex hull (mi_hull_above) beside two host solvers that give the same answers, in one process:

    python scripts/hull_timing.py [--out profiles/hull_timing.json] [--reps 30]

Cases: (a) 256 queries over 200 element sets against a bank of ~10^4 rows; (b) 256 queries of one 4-element system against 2000
candidates.  Per case: the two launches alone (device events around the enqueue, arrays resident), on the LDS path and with it forced
off; the whole `stability._run_kernel` (upload + call + read-back, host clock); the numpy restatement tests/hull_ref64.py; and, where
scipy is installed, scipy.optimize.linprog (HiGHS) looped over the queries.  Warm-up, then medians over `reps` calls with the spread
(min .. max); the kernel's answers are compared with the restatement's before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from matinvent_amd import stability as S  # noqa: E402
from tests import hull_ref64 as H  # noqa: E402


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


def case_many_sets(n_sets=200, n_queries=256, seed=0):
    """200 element sets of 2 .. 5 elements with 50 rows each (10^4 rows); query q belongs to set q % 200."""
    cases = [H.make_case(d=2 + g % 4, nc=50, seed=seed + g, nq=(n_queries - g + n_sets - 1) // n_sets, elems=None) for g in range(n_sets)]
    return H.merge_cases(cases)


def case_one_system(n_queries=256, seed=1):
    c = H.make_case(d=4, nc=2000, seed=seed, nq=n_queries, max_count=12)
    return c["bank"], H.one_group(c), c["query_c"], c["query_e"]


def linprog_loop(bank, groups, qc, qe):
    from scipy.optimize import linprog

    def run():
        out = np.full(len(qe), np.nan)
        for g in range(len(groups["grp_nelem"])):
            d = int(groups["grp_nelem"][g])
            X, E, _, _ = H.stage(bank, groups["grp_Z"][g][:d], groups["c_idx"][groups["grp_c_off"][g]:groups["grp_c_off"][g + 1]])
            fin = np.isfinite(E)
            for q in groups["q_idx"][groups["grp_q_off"][g]:groups["grp_q_off"][g + 1]]:
                out[q] = linprog(E[fin], A_eq=X[fin].T, b_eq=qc[q][:d], bounds=(0, None), method="highs").fun
        return out
    return run


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hull_timing.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "hull_timing.py measures on the GPU"
    results = []
    for name, (bank_arrays, groups, qc, qe) in (("256 queries over 200 element sets", case_many_sets()), ("256 queries of one 4-element system", case_one_system())):
        bank = S.PhaseBank(device="cuda")
        bank.add_rows([bank_arrays["Z"][i, :n] for i, n in enumerate(bank_arrays["nelem"])], [bank_arrays["frac"][i, :n] for i, n in enumerate(bank_arrays["nelem"])],
                      bank_arrays["energy"])
        want = H.run_call(bank_arrays, groups, qc, qe)
        call, stream = S.prepare_call(bank, groups, qc, qe), S.prepare_call(bank, groups, qc, qe, no_lds=True)
        for c in (call, stream):
            c.launch()
            got = c.read()
            assert all(np.array_equal(got[k], want[k], equal_nan=True) for k in S.OUTPUT_KEYS), name
        row = {"case": name, "queries": len(qe), "groups": len(groups["grp_nelem"]), "bank_rows": len(bank), "candidate_positions": len(groups["c_idx"]),
               "pivots_mean": float(want["iters"].mean()), "pivots_max": int(want["iters"].max()),
               "kernel": time_events(call.launch, args.reps), "kernel_no_lds": time_events(stream.launch, args.reps),
               "kernel_end_to_end": time_host(lambda: S._run_kernel(bank, groups, qc, qe), args.reps),
               "numpy_restatement": time_host(lambda: H.run_call(bank_arrays, groups, qc, qe), args.host_reps, sync=False)}
        try:
            lp = linprog_loop(bank_arrays, groups, qc, qe)
            assert np.abs(lp() - want["e_hull"]).max() < 1e-12
            row["scipy_linprog_loop"] = time_host(lp, args.host_reps, sync=False)
        except ImportError:
            row["scipy_linprog_loop"] = None
        results.append(row)
        print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
