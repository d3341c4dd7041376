"""Time fingerprint matching (mi_fp_match) against two baselines that give the same answers, in one process:

    python scripts/fp_match_timing.py [--out profiles/fp_match_timing.json] [--reps 30]

Cases: 256 queries (the rows of 20-atom crystals) of ONE formula at ncols = 192 and 384 against banks of 10^3, 10^4 and 10^5 rows; and 256
queries over 200 formulas against a bank of 4.5 10^4 rows.  Per case: the kernel call alone (device events around the enqueue, arrays
resident), the whole `_run_kernel` (plan + upload + call + read-back, host clock), a torch device matmul of the gathered rows with the same
reductions, and the per-pair host loop that memory._find uses, on a bounded sample of pairs and extrapolated.  Warm-up, then medians over
`reps` calls with the spread (min .. max); the answers of kernel and matmul are compared before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from matinvent_amd import novelty  # noqa: E402
from matinvent_amd.structure import FP_TOL, fingerprint_distance  # noqa: E402


def unit_rows(n, ncols, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, ncols, generator=g, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float().numpy()


def make_case(n_queries, n_formulas, bank_rows, ncols, seed=0):
    per = bank_rows // n_formulas
    rows = unit_rows(per * n_formulas, ncols, seed)
    query = np.zeros((n_queries, 2304), np.float32)
    query[:, :ncols] = unit_rows(n_queries, ncols, seed + 1)
    bank = novelty.FingerprintBank(device="cuda")
    formulas = [f"F{k // per}" for k in range(per * n_formulas)]
    bank.add_rows(formulas, [ncols] * len(formulas), rows, np.zeros(len(formulas), np.int64))
    qf = [f"F{k % n_formulas}" for k in range(n_queries)]
    groups = novelty.build_groups(qf, [ncols] * n_queries, np.zeros(n_queries, np.int64), bank)
    novelty.validate_groups(groups, n_queries, 2304, bank.host_len)
    return query, groups, bank


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


def time_host(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return spread(ts)


def matmul_baseline(query_dev, groups, bank, ncols, tol):
    """The same answers from torch: per group gather the candidate rows, one matmul, min / argmin / count."""
    ln = novelty.round4(ncols)
    mat = bank.rows[: bank.n_floats].view(-1, ln)                      # (every row of these cases has one length)
    q_off, c_off = groups["grp_q_off"], groups["grp_c_off"]
    q_idx, c_idx = torch.from_numpy(groups["q_idx"].astype(np.int64)).cuda(), torch.from_numpy(groups["c_idx"].astype(np.int64)).cuda()

    def run():
        best_d = torch.full((len(query_dev),), float("inf"), device="cuda")
        best_i = torch.full((len(query_dev),), -1, dtype=torch.int64, device="cuda")
        within = torch.zeros(len(query_dev), dtype=torch.int64, device="cuda")
        for g in range(len(groups["grp_ncols"])):
            qs, cs = q_idx[q_off[g]:q_off[g + 1]], c_idx[c_off[g]:c_off[g + 1]]
            d = 0.5 * (1.0 - query_dev[qs, :ln] @ mat[cs].T)
            m, a = d.min(dim=1)
            best_d[qs], best_i[qs], within[qs] = m, cs[a], (d <= tol).sum(dim=1)
        return best_d, best_i, within
    return run


def host_loop_estimate(query, groups, bank, sample=4000):
    """memory._find's loop: fingerprint_distance once per pair, in Python.  Timed on `sample` pairs, scaled to the call's pair count."""
    rows = bank.host_rows()
    g = np.random.default_rng(0)
    pairs = int((np.diff(groups["grp_q_off"]).astype(np.int64) * np.diff(groups["grp_c_off"]).astype(np.int64)).sum())
    qs, cs = g.integers(0, len(query), sample), g.integers(0, len(rows), sample)
    ln = len(rows[0])
    t = time.perf_counter()
    for q, c in zip(qs, cs):
        float(fingerprint_distance(rows[c], query[q, :ln])) <= FP_TOL
    per_pair = (time.perf_counter() - t) / sample
    return {"pairs": pairs, "sampled_pairs": sample, "per_pair_us": 1e6 * per_pair, "extrapolated_ms": 1e3 * per_pair * pairs}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fp_match_timing.json"))
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "fp_match_timing.py measures on the GPU"
    cases = [("one formula", 256, 1, m, n) for n in (192, 384) for m in (1000, 10000, 100000)] + [("200 formulas", 256, 200, 45000, 192)]
    results = []
    for name, nq, nf, m, ncols in cases:
        query, groups, bank = make_case(nq, nf, m, ncols)
        q_dev = torch.from_numpy(query).cuda()
        call = novelty.prepare_call(q_dev, groups, bank, FP_TOL)
        call.launch()
        bd, bi, nw, st, _ = call.read()
        base = matmul_baseline(q_dev, groups, bank, ncols, FP_TOL)
        md, mi_, mw = (t.cpu().numpy() for t in base())
        assert not st.any() and np.abs(bd - md).max() < 1e-5 and (nw == mw).all() and (bi == mi_).mean() > 0.99, name
        row = {"case": name, "queries": nq, "formulas": nf, "bank_rows": len(bank), "ncols": ncols, "work_items": int(call.args.n_items),
               "kernel": time_events(call.launch, args.reps),
               "kernel_end_to_end": time_host(lambda: novelty._run_kernel(query, groups, bank, FP_TOL), args.reps),
               "torch_matmul": time_events(base, args.reps),
               "torch_matmul_host_clock": time_host(base, args.reps),
               "host_loop": host_loop_estimate(query, groups, bank)}
        row["matmul_over_kernel"] = row["torch_matmul"]["median_ms"] / row["kernel"]["median_ms"]
        results.append(row)
        print(json.dumps(row), flush=True)
        del bank, call, q_dev
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "tol": FP_TOL, "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
