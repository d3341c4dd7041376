"""ms per mi_sym_refine call and per whole cell="given" chain (prepare -> find -> refine), medians of --repeats, on two workloads
of 256 crystals:
  random    20 atoms in 3 species at random positions in a triclinic cell (P1: one operation, the copy path);
  rocksalt  conventional rock-salt cells, every atom moved by at most 0.02 A and the cell strained by at most 0.002 an entry (192 operations
            of 8 atoms: every operation thread of the workgroup live).
Beside them the numpy restatement tests/refine_ref64.py per crystal on a bounded sample (--sample), whose outputs are compared bit for bit.
Writes profiles/refine_timing.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from matinvent_amd import matching, symmetry  # noqa: E402
from tests import refine_cases as RC  # noqa: E402
from tests import refine_ref64 as V  # noqa: E402
from tests import sm_cases as K  # noqa: E402
from tests import sm_ref64 as R  # noqa: E402
from tests import sym_ref64 as S  # noqa: E402


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


def workload(name, crystals, repeats, sample):
    off, types, frac, lat = K.batch(crystals)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = (t(off), t(types), t(frac), t(lat))
    tol = S.tolerances(off, lat, symmetry.SYMPREC)
    tol_d = torch.from_numpy(tol).cuda()
    prepared = matching.prepare_arrays(*args)
    find_ms, sym = timed(lambda: symmetry.find_symmetry_prepared(prepared, tol_d), repeats)
    refine_ms, ref = timed(lambda: symmetry.refine_prepared(prepared, args[1], args[2], args[3], sym), repeats)
    chain_ms, _ = timed(lambda: symmetry.refine_arrays(*args, tol_d), repeats)
    info, stat = ref.info.cpu().numpy(), ref.stat.cpu().numpy()
    sb = K.batch(crystals[:sample])
    P = R.prepare(*sb)
    F = S.find(P, tol[:sample], K.COS_TOL, margin=False)
    t0 = time.perf_counter()
    want = V.refine(P, sb[1], sb[2], sb[3], F)
    ref_ms = (time.perf_counter() - t0) * 1e3 / max(sample, 1)
    n = len(sb[1])
    equal = (np.array_equal(info[:sample], want["info"]) and np.array_equal(stat[:sample], want["stat"]) and np.array_equal(ref.frac.cpu().numpy()[:n], want["frac"]) and
             np.array_equal(ref.lat.cpu().numpy()[:sample], want["lat"]) and np.array_equal(ref.orbit.cpu().numpy()[:n], want["orbit"]) and
             np.array_equal(ref.trans_ref.cpu().numpy()[:sample], want["trans_ref"]))
    return {"workload": name, "crystals": len(crystals), "atoms": len(crystals[0][1]), "refine_ms": refine_ms, "chain_ms": chain_ms, "find_ms": find_ms,
            "refine_us_per_crystal": refine_ms * 1e3 / len(crystals), "chain_us_per_crystal": chain_ms * 1e3 / len(crystals),
            "n_ops": sorted(set(int(v) for v in info[:, 1])), "n_orbits": sorted(set(int(v) for v in info[:, 0])), "status_ok_frac": float((info[:, 7] == 0).mean()),
            "max_move_prepared_units": float(stat[:, 0].max()), "restatement_refine_ms_per_crystal": ref_ms, "restatement_sample": sample,
            "restatement_sample_equal_bits": bool(equal)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crystals", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--sample", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_timing.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    rand = [K.random_crystal(rng, [9, 4, 7]) for _ in range(a.crystals)]
    rock = [RC.perturb(rng, K.cell("rocksalt_conv")) for _ in range(a.crystals)]
    res = {"device": torch.cuda.get_device_name(0), "symprec": symmetry.SYMPREC, "angle_tol": symmetry.ANGLE_TOL, "repeats": a.repeats,
           "results": [workload("random", rand, a.repeats, a.sample), workload("rocksalt", rock, a.repeats, a.sample)]}
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
