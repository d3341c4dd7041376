"""ms per mi_sym_conventional call and per whole chain (prepare -> find -> primitive -> prepare -> find -> conventional), medians
of --repeats, on two workloads of 256 crystals:
  random    20 atoms in 3 species at random positions in a triclinic cell (P1: M = I, mult 1);
  rocksalt  primitive rock-salt cells with small displacements (48 operations; cF, mult 4, 8 atoms out).
Beside them the parent's chain on the same inputs (prepare -> find -> primitive, what primitive_records runs) and the numpy restatement
tests/conv_ref64.py per crystal on a bounded sample (--sample), whose conventional arrays are compared bit for bit.  Writes
profiles/conventional_timing.json."""
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
from tests import conv_ref64 as V  # noqa: E402
from tests import sm_cases as K  # noqa: E402
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
    parent_ms, (prim, _) = timed(lambda: symmetry.reduce_arrays(*args, tol_d), repeats)
    prepared = matching.prepare_arrays(prim.offsets, prim.types, prim.frac, prim.lat)
    find_ms, sym = timed(lambda: symmetry.find_symmetry_prepared(prepared, tol_d), repeats)
    conv_ms, conv = timed(lambda: symmetry.conventional_prepared(prepared, prim.types, prim.frac, prim.lat, sym), repeats)
    chain_ms, _ = timed(lambda: symmetry.conventional_arrays(*args, tol_d), repeats)
    info = conv.info.cpu().numpy()
    sb = K.batch(crystals[:sample])
    t0 = time.perf_counter()
    ch = V.chain(sb, symmetry.SYMPREC, K.COS_TOL, margin=False)
    chain_ref_ms = (time.perf_counter() - t0) * 1e3 / max(sample, 1)
    p = ch["prim"]
    t0 = time.perf_counter()
    ref = V.conventional(ch["P2"], p["types"], p["frac"], p["lat"], ch["F2"], margin=False)
    ref_ms = (time.perf_counter() - t0) * 1e3 / max(sample, 1)
    n = int(ref["conv_offsets"][-1])
    equal = (np.array_equal(info[:sample], ref["conv_info"]) and np.array_equal(conv.M.cpu().numpy()[:sample], ref["conv_M"]) and
             np.array_equal(conv.offsets.cpu().numpy()[:sample + 1], ref["conv_offsets"]) and np.array_equal(conv.frac.cpu().numpy()[:n], ref["frac"][:n]) and
             np.array_equal(conv.lat.cpu().numpy()[:sample], ref["lat"]))
    return {"workload": name, "crystals": len(crystals), "atoms": len(crystals[0][1]), "conventional_ms": conv_ms, "chain_ms": chain_ms,
            "parent_primitive_chain_ms": parent_ms, "second_find_ms": find_ms, "conventional_us_per_crystal": conv_ms * 1e3 / len(crystals),
            "chain_us_per_crystal": chain_ms * 1e3 / len(crystals), "bravais": sorted(set(V.BRAVAIS[i] for i in info[:, 0])),
            "status_ok_frac": float((info[:, 7] == 0).mean()), "atoms_out": int(conv.offsets[-1]), "restatement_conventional_ms_per_crystal": ref_ms,
            "restatement_chain_ms_per_crystal": chain_ref_ms, "restatement_sample": sample, "restatement_sample_equal_bits": bool(equal)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crystals", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--sample", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conventional_timing.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    rand = [K.random_crystal(rng, [9, 4, 7]) for _ in range(a.crystals)]
    L, z, f = K.cell("rocksalt_prim")
    rock = [(L, z, f + rng.normal(size=f.shape) * 0.001) for _ in range(a.crystals)]
    res = {"device": torch.cuda.get_device_name(0), "symprec": symmetry.SYMPREC, "angle_tol": symmetry.ANGLE_TOL, "repeats": a.repeats,
           "results": [workload("random", rand, a.repeats, a.sample), workload("rocksalt", rock, a.repeats, a.sample)]}
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
