"""in.extxyz out.npz: a structure bank for the device structure matcher (matching.StructureBank, UNFilter(matcher="structure",
reference_path=...)) from a user's own structures.  The .npz holds data only: atom counts, atomic numbers, float32 fractional
coordinates and cells, and the reduced formulas."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main(argv):
    if len(argv) != 3:
        print("usage: build_structure_bank.py in.extxyz out.npz", file=sys.stderr)
        return 2
    from matinvent_amd.matching import StructureBank
    from matinvent_amd.structure import read_extxyz
    records = read_extxyz(argv[1])
    bank = StructureBank.from_records(records, device="cpu")
    bank.save(argv[2])
    print(f"{len(bank)} structures, {len(bank.formulas)} formulas -> {argv[2]}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
