"""Turn a set of structures into a reference bank for the novelty filter (matinvent_amd.novelty):

    python scripts/build_fingerprint_bank.py train.extxyz bank.npz [--nbins 64] [--r-max 8.0] [--sigma 0.15] [--batch 4096]

Reads the extended-XYZ frames, computes their fingerprints on the GPU in batches, and writes the .npz that UNFilter(reference_path=...)
and FingerprintBank.load take."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from matinvent_amd.novelty import FingerprintBank  # noqa: E402
from matinvent_amd.structure import FP_NBINS, FP_R_MAX, FP_SIGMA, read_extxyz  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("extxyz")
    ap.add_argument("out")
    ap.add_argument("--nbins", type=int, default=FP_NBINS)
    ap.add_argument("--r-max", type=float, default=FP_R_MAX)
    ap.add_argument("--sigma", type=float, default=FP_SIGMA)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    records = read_extxyz(args.extxyz)
    bank = FingerprintBank(nbins=args.nbins, r_max=args.r_max, sigma=args.sigma, device=args.device)
    for at in range(0, len(records), args.batch):
        bank.add(records[at:at + args.batch])
    bank.save(args.out)
    print(f"{len(records)} structures -> {len(bank)} rows of {len(bank.formulas)} formulas "
          f"({sum(bank.flagged.values())} flagged, kept by formula) in {args.out}")
    return bank


if __name__ == "__main__":
    main()
