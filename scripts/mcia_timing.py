"""ms per substrate-matching call for 256 random cells of the size of a 20-atom crystal (edges 4.5 .. 9 A, angles 70 .. 110
degrees), film_max_miller = 1:
  si100        against Si (100) alone, lowest mode;
  bank         against a bank of 9 substrates x 13 planes (cubic, hexagonal and tetragonal cells of common substrate sizes), lowest mode;
  bank_count   the same bank in count mode (every match counted, the least strained one kept).
A call is planes + search + reduce on device tensors (substrates.match_arrays), the bank's tables built beforehand and timed apart.
Beside the numpy restatement tests/zsl_ref64.py on a bounded sample of the same films (--sample), whose integers and areas are compared
bit for bit.  A record, not a pass criterion.  Writes profiles/mcia_timing.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from matinvent_amd import substrates  # noqa: E402
from tests import zsl_cases as Z  # noqa: E402
from tests import zsl_ref64 as R  # noqa: E402

CUBIC = {"Si": 5.4437, "GaAs": 5.653, "InP": 5.869, "MgO": 4.212, "SrTiO3": 3.905}
HEXAGONAL = {"GaN": (3.189, 5.185), "ZnO": (3.250, 5.207), "Al2O3": (4.759, 12.991)}
TETRAGONAL = {"TiO2": (4.594, 2.959)}


def bank_cells():
    cells = [(k, Z.cubic(a)) for k, a in CUBIC.items()]
    cells += [(k, Z.cell([a, a, c], [90.0, 90.0, 120.0])) for k, (a, c) in HEXAGONAL.items()]
    cells += [(k, Z.cell([a, a, c], [90.0] * 3)) for k, (a, c) in TETRAGONAL.items()]
    return cells


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out


def workload(name, films, bank_spec, count, repeats, sample):
    zsl = substrates.ZSL()
    subs = [substrates.Substrate(k, lat.reshape(3, 3), hk) for k, lat, hk in bank_spec]
    bank_ms, bank = timed(lambda: substrates.SubstrateBank(subs, zsl), repeats)
    lat = torch.from_numpy(films).cuda()
    call_ms, res = timed(lambda: substrates.match_arrays(zsl, lat, bank, count), repeats)
    t0 = time.perf_counter()
    res._host = None
    status = res.mcia_status
    read_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ref = R.analyze(films[:sample], R.planes(1), [(l, hk if hk is not None else R.planes(1)) for _, l, hk in bank_spec], None, count)
    ref_ms = (time.perf_counter() - t0) * 1e3 / max(sample, 1)
    d, r, n = res.res_d.cpu().numpy()[:sample], res.res_i.cpu().numpy()[:sample], res.res_n.cpu().numpy()[:sample]
    equal = (np.array_equal(r, ref["res_i"]) and np.array_equal(n, ref["res_n"]) and np.array_equal(d[..., 0], ref["res_d"][..., 0]) and
             np.array_equal(res.mcia[:sample], ref["mcia"]))
    out = {"workload": name, "films": len(films), "substrates": bank.S, "substrate_planes": bank.Ps, "film_planes": 13, "items": len(films) * 13 * bank.Ps,
           "count": bool(count), "bank_build_ms": bank_ms, "call_ms": call_ms, "us_per_film": call_ms * 1e3 / len(films), "read_ms": read_ms,
           "status_ok_frac": float((status == 0).mean()), "status_no_match_frac": float((status == 1).mean()), "mean_mcia_of_ok": float(np.mean(res.mcia[status == 0])) if (status == 0).any() else None,
           "restatement_ms_per_film": ref_ms, "restatement_sample": sample, "restatement_sample_equal_bits": bool(equal),
           "restatement_over_device_per_film": ref_ms / (call_ms / len(films)), "restatement_margin": ref["margin"]}
    if count:
        out["mean_matches_per_film_and_plane"] = float(res.n_matches.mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--films", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sample", type=int, default=4, help="films the restatement runs on against Si (100); the bank workloads take a quarter of it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcia_timing.json"))
    args = ap.parse_args()
    films = Z.triclinic(2024, args.films)
    si = [("Si", Z.cubic(CUBIC["Si"]), [(1, 0, 0)])]
    bank = [(k, lat, None) for k, lat in bank_cells()]
    few = max(1, args.sample // 4)
    rows = [workload("si100", films, si, False, args.repeats, args.sample), workload("bank", films, bank, False, args.repeats, few),
            workload("bank_count", films, bank, True, args.repeats, few)]
    doc = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "workloads": rows}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
