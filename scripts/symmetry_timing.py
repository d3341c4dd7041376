"""ms per mi_sym_find and mi_sym_primitive call on two workloads of 256 crystals:
  random   20 atoms in 3 species at random positions in a triclinic cell (P1: two maps, one operation);
  cubic    conventional rock-salt cells with small displacements (the heavy case: 48 maps x 4 translations, 192 operations, 4 pure
           translations, a primitive cell of 2 atoms).
Beside the numpy restatement tests/sym_ref64.py on a bounded sample of the same crystals (--sample), whose outputs are compared bit for
bit.  Writes profiles/symmetry_timing.json."""
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
    prep_ms, prepared = timed(lambda: matching.prepare_arrays(*args), repeats)
    find_ms, sym = timed(lambda: symmetry.find_symmetry_prepared(prepared, tol), repeats)
    prim_ms, prim = timed(lambda: symmetry.primitive_arrays(prepared, *args[1:], sym), repeats)
    info = sym.host()
    sub = crystals[:sample]
    sb = K.batch(sub)
    t0 = time.perf_counter()
    P = R.prepare(*sb)
    F = S.find(P, tol[:sample], K.COS_TOL, margin=False)
    Pm = S.primitive(P, sb[1], sb[2], sb[3], F, margin=False)
    ref_ms = (time.perf_counter() - t0) * 1e3 / max(sample, 1)
    n = int(Pm["prim_offsets"][-1])
    equal = (np.array_equal(info[:sample], F["info"]) and np.array_equal(sym.rot_hist.cpu().numpy()[:sample], F["rot_hist"]) and
             np.array_equal(prim.offsets.cpu().numpy()[:sample + 1], Pm["prim_offsets"]) and np.array_equal(prim.frac.cpu().numpy()[:n], Pm["frac"][:n]))
    return {"workload": name, "crystals": len(crystals), "atoms": len(crystals[0][1]), "prepare_ms": prep_ms, "find_ms": find_ms, "primitive_ms": prim_ms,
            "us_per_crystal": (find_ms + prim_ms) * 1e3 / len(crystals), "mean_maps": float(info[:, 2].mean()), "mean_ops": float(info[:, 0].mean()),
            "mean_trans": float(info[:, 1].mean()), "status_ok_frac": float((info[:, 7] == 0).mean()), "primitive_atoms": int(prim.offsets[-1]),
            "restatement_ms_per_crystal": ref_ms, "restatement_sample": sample, "restatement_sample_equal_bits": bool(equal)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crystals", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--sample", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "symmetry_timing.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    rand = [K.random_crystal(rng, [9, 4, 7]) for _ in range(a.crystals)]
    L, z, f = K.cell("rocksalt_conv")
    cubic = [(L, z, f + rng.normal(size=f.shape) * 0.001) for _ in range(a.crystals)]
    res = {"device": torch.cuda.get_device_name(0), "symprec": symmetry.SYMPREC, "angle_tol": symmetry.ANGLE_TOL,
           "results": [workload("random", rand, a.repeats, a.sample), workload("cubic", cubic, a.repeats, a.sample)]}
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
