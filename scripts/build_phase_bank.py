"""Turn a set of structures with energies into a phase bank for the stability filter (matinvent_amd.stability):

    python scripts/build_phase_bank.py in.extxyz out.npz [--energy-key energy] [--total] [--predictor DIR --task NAME] [--batch 64]

The energies come from each frame's info field `--energy-key` (per atom; --total: per cell), or from a saved PropertyPredictor
(--predictor, a save_predictor directory; --task, the property that is the energy per atom) evaluated on the structures: such a bank is
consistent with the energies relax.Relaxer returns for the same predictor.  Writes the .npz that SUNFilter(phase_path=...) and
PhaseBank.load take; the file holds data only (element lists, fractions, energies)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from matinvent_amd.stability import PhaseBank  # noqa: E402
from matinvent_amd.structure import read_extxyz  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("extxyz")
    ap.add_argument("out")
    ap.add_argument("--energy-key", default="energy")
    ap.add_argument("--total", action="store_true", help="the info field is the energy of the cell, not per atom")
    ap.add_argument("--predictor", default=None)
    ap.add_argument("--task", default=None)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    records = read_extxyz(args.extxyz)
    if args.predictor:
        if not args.task:
            ap.error("--predictor needs --task (the name of the property that is the energy per atom)")
        from matinvent_amd.rewards import Surrogate
        energies, per_atom = Surrogate(model_path=args.predictor, task=args.task, batch_size=args.batch, device=args.device).calc(records), True
    else:
        missing = [i for i, r in enumerate(records) if args.energy_key not in r.info]
        if missing:
            raise SystemExit(f"{args.extxyz}: frame {missing[0]} (and {len(missing) - 1} more) has no info field {args.energy_key!r}")
        energies, per_atom = np.array([float(r.info[args.energy_key]) for r in records], np.float64), not args.total
    bank = PhaseBank(device=args.device)
    bank.add(records, energies, per_atom=per_atom)
    bank.save(args.out)
    systems = {tuple(bank.Z[i, :bank.nelem[i]]) for i in range(len(bank))}
    print(f"{len(records)} structures -> {len(bank)} rows over {len(systems)} element sets ({bank.dropped} with more than 8 elements dropped, "
          f"{int(np.isnan(bank.energy).sum())} without a finite energy) in {args.out}")
    return bank


if __name__ == "__main__":
    main()
