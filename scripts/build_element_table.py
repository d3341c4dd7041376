"""Write the element table of matinvent_amd.chemistry.ElementTable from the user's own data files -- no table is shipped:

    python scripts/build_element_table.py --oxidation-states ox.txt --properties props.csv --metals metals.txt --out elements.json

--oxidation-states  text: a symbol, then its integer oxidation states, per line; `#` starts a comment; a symbol alone has an empty list
                    (the shape of SMACT's oxidation-state files, [UPSTREAM-UNVERIFIED]).  A symbol listed twice is refused.
--properties        CSV with a header naming the columns symbol, eneg (Pauling electronegativity), abundance (crustal, ppm); an empty
                    cell is a missing value.  Elements that appear only here are written with an empty list of states.
--metals            text: the symbols of the metals, separated by white space or commas; `#` starts a comment.
The result is loaded once through ElementTable, so every refusal of the loader (unknown symbols, duplicate or out-of-range states, lists
longer than 32, non-finite electronegativities) is raised here, by name, before the file is written."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def strip(line):
    return line.split("#", 1)[0].strip()


def read_states(path):
    out = {}
    with open(path) as f:
        for n, line in enumerate(f, 1):
            words = strip(line).replace(",", " ").split()
            if not words:
                continue
            if words[0] in out:
                raise ValueError(f"{path}:{n}: {words[0]} is listed twice")
            try:
                out[words[0]] = [int(w) for w in words[1:]]
            except ValueError:
                raise ValueError(f"{path}:{n}: {words[0]}: an oxidation state is not an integer: {words[1:]}") from None
    return out


def read_properties(path):
    out = {}
    with open(path, newline="") as f:
        rows = csv.DictReader(line for line in f if strip(line))
        if rows.fieldnames is None or "symbol" not in [c.strip() for c in rows.fieldnames]:
            raise ValueError(f"{path}: the header must name the columns symbol, eneg, abundance")
        for row in rows:
            row = {k.strip(): (v or "").strip() for k, v in row.items() if k}
            value = lambda k: float(row[k]) if row.get(k) else None
            out[row["symbol"]] = (value("eneg"), value("abundance"))
    return out


def read_metals(path):
    with open(path) as f:
        return {w for line in f for w in strip(line).replace(",", " ").split()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--oxidation-states", required=True)
    ap.add_argument("--properties", required=True)
    ap.add_argument("--metals", required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    states, props, metals = read_states(args.oxidation_states), read_properties(args.properties), read_metals(args.metals)
    elements = {}
    for sym in list(states) + [s for s in props if s not in states]:
        eneg, abundance = props.get(sym, (None, None))
        elements[sym] = {"ox": states.get(sym, []), "eneg": eneg, "metal": sym in metals, "abundance": abundance}
    unknown = sorted(metals - set(elements))
    if unknown:
        raise ValueError(f"{args.metals}: metals without a row in the other files: {unknown}")
    from matinvent_amd.chemistry import ElementTable
    ElementTable(elements)   # the loader's refusals, before anything is written
    with open(args.out, "w") as f:
        json.dump({"elements": elements}, f, indent=1)
    print(f"wrote {args.out}: {len(elements)} elements, {sum(1 for e in elements.values() if e['ox'])} with oxidation states, {len(metals)} metals")


if __name__ == "__main__":
    main()
