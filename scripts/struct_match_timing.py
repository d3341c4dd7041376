"""ms per mi_sm_prepare and mi_sm_match call on two synthetic workloads of 20-atom crystals in 3 species, every pair a full
evaluation (bank rows and queries are strained, displaced, permuted copies of their formula's prototype):
  A  256 queries over 200 formulas against a bank of 4.5e4 structures (225 per formula);
  B  256 queries of one formula against 1e4 candidates (--b-candidates).
Beside the numpy restatement tests/sm_ref64.py on a bounded sample of pairs (--sample), with the mean maps and items per pair.  Writes
profiles/struct_match_timing.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from matinvent_amd import matching  # noqa: E402
from tests import sm_cases as K  # noqa: E402
from tests import sm_ref64 as R  # noqa: E402


def variants(rng, proto, count):
    L, z, f = proto
    out = []
    for _ in range(count):
        strain = np.eye(3) + rng.uniform(-0.03, 0.03, (3, 3))
        out.append(K.transformed(rng, (L @ strain, z, f), sigma=0.02))
    return out


def device_set(crystals):
    off, types, frac, lat = K.batch(crystals)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = (t(off), t(types), t(frac), t(lat))
    return args, matching.prepare_arrays(*args)


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b))
    return float(np.median(best)), out


def workload(name, rng, formulas, per_formula, queries, repeats, sample):
    protos = [K.random_crystal(rng, c, s) for c, s in formulas]
    bank, rows = [], []
    for p in protos:
        rows.append(range(len(bank), len(bank) + per_formula))
        bank += variants(rng, p, per_formula)
    owner = [i % len(protos) for i in range(queries)]
    qs = [variants(rng, protos[o], 1)[0] for o in owner]
    bargs, _ = device_set(bank)
    qargs, _ = device_set(qs)
    prep_ms, B = timed(lambda: matching.prepare_arrays(*bargs), repeats)
    _, Q = timed(lambda: matching.prepare_arrays(*qargs), 1)
    pairs = torch.tensor([(i, r) for i, o in enumerate(owner) for r in rows[o]], dtype=torch.int32, device="cuda")
    match_ms, out = timed(lambda: matching.match_pairs(Q, B, pairs), repeats)
    st = out["status"].cpu().numpy()
    res = {"workload": name, "queries": queries, "bank": len(bank), "pairs": int(len(pairs)), "prepare_bank_ms": prep_ms, "match_ms": match_ms,
           "us_per_pair": 1e3 * match_ms / len(pairs), "status_ok_frac": float((st == 0).mean()), "fit_frac": float(out["fit"].float().mean()),
           "mean_maps": float(out["n_maps"].float().mean()), "mean_items": float(out["n_items"].float().mean())}
    # the restatement on a bounded sample
    PB, PQ = R.prepare(*K.batch(bank[:per_formula])), R.prepare(*K.batch([q for q, o in zip(qs, owner) if o == 0][:1]))
    t0, same = time.perf_counter(), True
    for c in range(min(sample, per_formula)):
        r = R.match_pair(PQ, 0, PB, c, 0.2, K.COS_TOL)
        same = same and r["rms"] == float(out["rms"][c])
    res["restatement_ms_per_pair"] = 1e3 * (time.perf_counter() - t0) / min(sample, per_formula)
    res["restatement_sample_equal_bits"] = bool(same)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sample", type=int, default=8)
    ap.add_argument("--a-formulas", type=int, default=200)
    ap.add_argument("--a-per-formula", type=int, default=225)
    ap.add_argument("--b-candidates", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "struct_match_timing.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    elements = list(range(3, 90))
    formulas = []
    for _ in range(args.a_formulas):
        a = int(rng.integers(2, 9))
        b = int(rng.integers(2, 19 - a - 1))
        formulas.append(([a, b, 20 - a - b], [int(e) for e in sorted(rng.choice(elements, 3, replace=False))]))
    results = [workload("A", rng, formulas, args.a_per_formula, 256, args.repeats, args.sample),
               workload("B", rng, [([9, 4, 7], [3, 8, 26])], args.b_candidates, 256, args.repeats, args.sample)]
    doc = {"device": torch.cuda.get_device_name(0), "atoms": 20, "ltol": 0.2, "stol": 0.3, "angle_tol": 5.0, "results": results,
           "kernels": {"sm_prepare_kernel": {"vgprs": 62, "lds_bytes": 68, "scratch": 0},
                       "sm_match_kernel<32>": {"vgprs": 135, "lds_bytes": 51520, "scratch": 0},
                       "sm_match_kernel<64>": {"vgprs": 133, "lds_bytes": 159040, "scratch": 0}},
           "not_measured": ["mi_fp_match on the same sets"]}
    for r in results:
        print(json.dumps(r), flush=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
