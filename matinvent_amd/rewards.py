"""Rewards with the `Reward.scoring` return contract (rewards/reward.py:8-115 returns (rewards, prop_dict, failed_mask)): the synthetic
reward that benchmarks and smoke runs use, the reference's scalarisation `Reward`, and the calculators that run on this library --
`Surrogate` (a trained property predictor), `EAboveHull` (the energy above the convex hull), `HeatCapacity` (the
harmonic heat capacity of a predictor read as an energy, the reference's rewards/calculators/fairchem/phonon.py; DESIGN 47, and from a q-mesh with method="mesh": DESIGN 51), `Elastic`
(the bulk, shear and Young's modulus, Poisson's ratio and the Pugh ratio from the elastic tensor of a predictor read as an energy, the
reference's rewards/calculators/fairchem/elastic.py), `Symmetry` (the operation count, point-group order or crystal system of
the symmetry finder) and `PyMatGen` (density, HHI, and the minimal coincident interface area on a substrate: DESIGN 52).  The energies behind EAboveHull,
HeatCapacity and Elastic are a PropertyPredictor's, relaxed by relax.Relaxer: the reference's MLIP calculators (MatterSim, fairchem) themselves, ALIGNN and DFT stay out of scope (SURVEY.md section 2 rows
11-12)."""
import numpy as np


class SyntheticReward:
    def __init__(self, root_dir="rewards", reward_threshold=0.8, seed=7, mode="uniform", n_props=1, reduce="mean", **kwargs):
        assert reduce in ("mean", "min")
        self.root_dir, self.threshold, self.mode = root_dir, reward_threshold, mode
        self.n_props, self.reduce = int(n_props), reduce
        self.rng = np.random.default_rng(seed)

    def scoring(self, samples, label="tmp"):
        strucs = samples[0] if isinstance(samples, tuple) else samples
        n = len(strucs)
        if self.mode == "light":  # a deterministic structure-dependent score: prefers light elements
            z = np.array([np.mean(getattr(s, "species", [50])) for s in strucs], dtype=float)
            r = np.clip(1.0 - z / 94.0, 0.0, 1.0)
        else:
            r = self.rng.random(n)
        props = {"synthetic": r.copy()}
        for k in range(1, self.n_props):  # multi-objective (BASELINE config 5): extra columns, reduced like rewards/reward.py:102-106
            props[f"synthetic_{k}"] = self.rng.random(n)
        cols = np.stack(list(props.values()))
        r = cols.mean(axis=0) if self.reduce == "mean" else cols.min(axis=0)
        return r, props, np.zeros(n, dtype=bool)


def linear_scaling(values, minv=0.0, maxv=6.0):
    """rewards/reward.py:8-12: (v - minv) / (maxv - minv) clipped to [0, 1]."""
    ss = (np.asarray(values, dtype=float) - minv) / (maxv - minv)
    return np.clip(ss, 0.0, 1.0)


class Reward:
    """rewards/reward.py:33-115 -- the scalarisation the RL loop ranks samples with: every property is mapped to [0, 1] by
    `linear_scaling` in one of three modes (`ascending`; `descending` = scale -v between -maxv and -minv; a float target = scale
    -|v - target| the same way), the scaled columns are reduced (`mean` / `min` / `weight`: weighted sum), and samples for which
    any calculator returned NaN get reward 0 and are reported in the failed mask.  `prop_cfg` entries need `name`, `calculator`
    (an object with `.calc(samples, label) -> array`), `target`, `minv`, `maxv` (+ `weight`)."""

    def __init__(self, root_dir, prop_cfg, reward_threshold, reduce="mean", **kwargs):
        assert reduce in ("mean", "min", "weight")
        self.root_dir, self.prop_cfg, self.threshold, self.reduce, self.cfg = root_dir, prop_cfg, reward_threshold, reduce, kwargs
        import os
        os.makedirs(self.root_dir, exist_ok=True)

    @staticmethod
    def _get(cfg, key):
        return cfg[key] if isinstance(cfg, dict) or hasattr(cfg, "__getitem__") and not hasattr(cfg, key) else getattr(cfg, key)

    def calc_props(self, samples, label="tmp"):
        prop_dict, raw = {}, []
        for c in self.prop_cfg:
            p = np.asarray(self._get(c, "calculator").calc(samples, label), dtype=float)
            raw.append(p)
            prop_dict[self._get(c, "name")] = np.nan_to_num(p, nan=0.0).astype(float)
        return prop_dict, np.isnan(np.array(raw)).any(axis=0)

    def scoring(self, samples, label="tmp"):
        prop_dict, failed = self.calc_props(samples, label)
        scaled = {}
        for c in self.prop_cfg:
            name, target, minv, maxv = (self._get(c, k) for k in ("name", "target", "minv", "maxv"))
            if target == "ascending":
                scaled[name] = linear_scaling(prop_dict[name], minv, maxv)
            elif target == "descending":
                scaled[name] = linear_scaling(-prop_dict[name], -maxv, -minv)
            elif isinstance(target, float):
                scaled[name] = linear_scaling(-np.abs(prop_dict[name] - target), -maxv, -minv)
            else:
                raise TypeError("prop cfg.target must be a float or descending or ascending")
        cols = np.array(list(scaled.values()))
        if self.reduce == "mean":
            rewards = cols.mean(axis=0)
        elif self.reduce == "min":
            rewards = cols.min(axis=0)
        else:
            rewards = np.array([scaled[self._get(c, "name")] * self._get(c, "weight") for c in self.prop_cfg]).sum(axis=0)
        rewards[failed] = 0.0
        return rewards, prop_dict, failed


class Surrogate:
    """A trained property predictor (predictor.PropertyPredictor) as a calculator of `Reward.prop_cfg`: `.calc(samples, label)`
    returns the de-normalised prediction of property `task` per structure, NaN for a structure the predictor cannot evaluate (-> failed ->
    reward 0).  model_path: a directory written by predictor.save_predictor, loaded on first use; or predictor: a loaded model (anything
    with `.names` and `.predict(records, batch_size=) -> [n][P]`).  An unknown `task` is a ValueError as soon as the names are known."""

    def __init__(self, root_dir="rewards", model_path=None, predictor=None, task=None, batch_size=64, device=None, **kwargs):
        if (model_path is None) == (predictor is None):
            raise ValueError("Surrogate: give exactly one of model_path (a save_predictor directory) and predictor (a loaded model)")
        if task is None:
            raise ValueError("Surrogate: task (the name of the property to return) is required")
        self.root_dir, self.model_path, self.task, self.batch_size, self.device = root_dir, model_path, str(task), int(batch_size), device
        self.predictor = None
        if predictor is not None:
            self._adopt(predictor)
        elif model_path is not None:
            from .predictor import read_hparams
            self._column(read_hparams(model_path)["names"])   # (the names are in hparams.yaml: an unknown task is refused before any weight is read)

    def _column(self, names):
        names = [str(n) for n in names]
        if self.task not in names:
            raise ValueError(f"Surrogate: unknown property name {self.task!r}: the predictor has {names}")
        return names.index(self.task)

    def _adopt(self, predictor):
        self.col = self._column(predictor.names)
        self.predictor = predictor

    def calc(self, samples, label="tmp"):
        strucs = samples[0] if isinstance(samples, tuple) else samples
        if self.predictor is None:
            from .predictor import load_predictor
            self._adopt(load_predictor(self.model_path, device=self.device))
        if len(strucs) == 0:
            return np.zeros(0, dtype=float)
        y = np.asarray(self.predictor.predict(list(strucs), batch_size=self.batch_size), dtype=float).reshape(len(strucs), -1)
        return y[:, self.col].copy()


class EAboveHull:
    """The energy above the convex hull (stability.energy_above_hull) as a calculator of `Reward.prop_cfg`: `.calc(samples,
    label)` returns e_above in eV/atom per structure, NaN where the solver did not end at an optimum or the structure has no energy (->
    failed -> reward 0); target "descending" then optimises towards stability.  bank: a stability.PhaseBank, or phase_path: a .npz of
    scripts/build_phase_bank.py, loaded on first use.  The energies are the second member of `samples` when it is a tuple (strucs,
    energies); otherwise relaxer(strucs, None) -> (strucs, energies) supplies them (relax.Relaxer, whose energies the bank must match)."""

    def __init__(self, bank=None, phase_path=None, relaxer=None, per_atom=True, root_dir="rewards", device="cuda", **kwargs):
        if (bank is None) == (phase_path is None):
            raise ValueError("EAboveHull: give exactly one of bank (a stability.PhaseBank) and phase_path (a .npz phase bank)")
        self.bank, self.phase_path, self.relaxer, self.per_atom, self.root_dir, self.device = bank, phase_path, relaxer, bool(per_atom), root_dir, device

    def calc(self, samples, label="tmp"):
        from . import stability
        strucs, energies = (samples[0], samples[1] if len(samples) > 1 else None) if isinstance(samples, tuple) else (samples, None)
        if len(strucs) == 0:
            return np.zeros(0, dtype=float)
        if energies is None:
            if self.relaxer is None:
                raise ValueError("EAboveHull: no energies -- pass samples as (strucs, energies) or give relaxer (relax.Relaxer)")
            strucs, energies = self.relaxer(list(strucs), None)
        if self.bank is None:
            self.bank = stability.PhaseBank.load(self.phase_path, device=self.device)
        res = stability.energy_above_hull(list(strucs), energies, self.bank, self.per_atom)
        return np.where(res["status"] == stability.OK, res["e_above"], np.nan).astype(float)


class HeatCapacity:
    """The harmonic heat capacity (vibrations.analyze_records) as a calculator of `Reward.prop_cfg`: `.calc(samples, label)`
    returns c_v at `temperature` in J / K / g per structure -- the Gamma-point modes of property `task` of a predictor read as an energy
    (eV; per atom with per_atom).  NaN (-> failed -> reward 0) on any status other than OK and, with require_stable, for a structure with
    an imaginary mode.  predictor: a loaded PropertyPredictor, or model_path: a directory written by predictor.save_predictor, loaded on
    first use.  relaxer (relax.Relaxer, or any strucs, path -> (strucs, energies)): the structures are relaxed first, as the reference
    does.  The remaining keywords are vibrations.Vibrations' (delta, nu_cut, batch_size, supercell, det_min).
    method = "mesh" (phonons.analyze_records) takes the heat capacity per primitive cell from a q-mesh instead: the supercell
    ((a, b, c), or "auto" with min_length) is built around a displaced home cell, mesh = (m_a, m_b, m_c) is the Gamma-centred grid, the
    remaining keywords are phonons.Phonons' (tie_tol and workspace_cap too), and require_stable fails a structure with an imaginary mode
    anywhere on the mesh.  method = "gamma", the default, is the Gamma-point path above, unchanged."""

    def __init__(self, root_dir="rewards", predictor=None, model_path=None, task=None, temperature=300.0, relaxer=None, require_stable=False,
                 supercell=(1, 1, 1), per_atom=True, device=None, method="gamma", mesh=(4, 4, 4), min_length=10.0, **kwargs):
        if method not in ("gamma", "mesh"):
            raise ValueError(f"HeatCapacity: method = {method!r}: \"gamma\" or \"mesh\"")
        self.method = method
        if (model_path is None) == (predictor is None):
            raise ValueError("HeatCapacity: give exactly one of model_path (a save_predictor directory) and predictor (a loaded model)")
        if task is None:
            raise ValueError("HeatCapacity: task (the name of the property read as the energy) is required")
        if not (np.isfinite(float(temperature)) and float(temperature) > 0):
            raise ValueError(f"HeatCapacity: temperature = {temperature}: must be finite and positive")
        self.root_dir, self.model_path, self.predictor, self.task, self.device = root_dir, model_path, predictor, str(task), device
        self.temperature, self.relaxer, self.require_stable = float(temperature), relaxer, bool(require_stable)
        if method == "mesh":
            self.vib_kw = dict(kwargs, supercell=supercell if isinstance(supercell, str) else tuple(int(r) for r in supercell), per_atom=bool(per_atom),
                               mesh=tuple(int(r) for r in mesh), min_length=float(min_length))
        else:
            self.vib_kw = dict(kwargs, supercell=tuple(int(r) for r in supercell), per_atom=bool(per_atom))
        self.vib, self.last = None, None
        if predictor is not None:
            self._analysis()
        else:
            from .predictor import read_hparams
            names = [str(n) for n in read_hparams(model_path)["names"]]
            if self.task not in names:
                raise ValueError(f"HeatCapacity: unknown property name {self.task!r}: the predictor has {names}")

    def _analysis(self):
        if self.vib is None:
            from .vibrations import Vibrations
            if self.predictor is None:
                from .predictor import load_predictor
                self.predictor = load_predictor(self.model_path, device=self.device)
            if self.method == "mesh":
                from .phonons import Phonons
                self.vib = Phonons(self.predictor, self.task, temperatures=(self.temperature,), **self.vib_kw)
            else:
                self.vib = Vibrations(self.predictor, self.task, temperatures=(self.temperature,), **self.vib_kw)
        return self.vib

    def calc(self, samples, label="tmp"):
        from . import vibrations
        strucs = samples[0] if isinstance(samples, tuple) else samples
        if len(strucs) == 0:
            return np.zeros(0, dtype=float)
        if self.relaxer is not None:
            strucs, _ = self.relaxer(list(strucs), None)
        if self.method == "mesh":
            from . import phonons
            res = phonons.analyze_records(self._analysis(), list(strucs))
        else:
            res = vibrations.analyze_records(self._analysis(), list(strucs))
        self.last = res
        out = np.where(res["status"] == 0, res["c_v_gram"][:, 0], np.nan).astype(float)
        if self.require_stable:
            out[res["n_imag"] > 0] = np.nan
        return out


class Elastic:
    """An elastic modulus (elasticity.analyze_records) as a calculator of `Reward.prop_cfg`: `.calc(samples, label)` returns
    `quantity` -- bulk_modulus, shear_modulus, young_modulus (GPa), poisson_ratio or pugh_ratio -- in the `average` voigt, reuss or hill
    per structure, from the elastic tensor of property `task` of a predictor read as an energy (eV; per atom with per_atom).  "voigt" is
    the default because the reference's script returns bulk_modulus.voigt.  NaN (-> failed -> reward 0) on BAD_INPUT; for the Reuss and Hill
    averages also on SINGULAR and when cond > cond_max (1e12: a stated, untuned choice -- the device applies no threshold); with
    require_stable also when C has a negative eigenvalue (Born stability).  predictor: a loaded PropertyPredictor, or model_path: a
    directory written by predictor.save_predictor, loaded on first use.  relaxer (relax.Relaxer, or any strucs, path -> (strucs,
    energies)): the structures are relaxed first, as the reference does.  The remaining keywords are elasticity.Elasticity's (delta,
    ion_steps, relax, batch_size, det_min)."""
    QUANTITIES = ("bulk_modulus", "shear_modulus", "young_modulus", "poisson_ratio", "pugh_ratio")
    AVERAGES = ("voigt", "reuss", "hill")

    def __init__(self, root_dir="rewards", predictor=None, model_path=None, task=None, quantity="bulk_modulus", average="voigt", relaxer=None,
                 require_stable=False, cond_max=1e12, per_atom=True, device=None, **kwargs):
        if (model_path is None) == (predictor is None):
            raise ValueError("Elastic: give exactly one of model_path (a save_predictor directory) and predictor (a loaded model)")
        if task is None:
            raise ValueError("Elastic: task (the name of the property read as the energy) is required")
        if quantity not in self.QUANTITIES:
            raise ValueError(f"Elastic: quantity = {quantity!r}: one of {self.QUANTITIES}")
        if average not in self.AVERAGES:
            raise ValueError(f"Elastic: average = {average!r}: one of {self.AVERAGES}")
        if not float(cond_max) > 0:
            raise ValueError(f"Elastic: cond_max = {cond_max}: must be positive")
        self.root_dir, self.model_path, self.predictor, self.task, self.device = root_dir, model_path, predictor, str(task), device
        self.quantity, self.average, self.relaxer = str(quantity), str(average), relaxer
        self.require_stable, self.cond_max = bool(require_stable), float(cond_max)
        self.ela_kw = dict(kwargs, per_atom=bool(per_atom))
        self.ela, self.last = None, None
        if predictor is not None:
            self._analysis()
        else:
            from .predictor import read_hparams
            names = [str(n) for n in read_hparams(model_path)["names"]]
            if self.task not in names:
                raise ValueError(f"Elastic: unknown property name {self.task!r}: the predictor has {names}")

    def _analysis(self):
        if self.ela is None:
            from .elasticity import Elasticity
            if self.predictor is None:
                from .predictor import load_predictor
                self.predictor = load_predictor(self.model_path, device=self.device)
            self.ela = Elasticity(self.predictor, self.task, **self.ela_kw)
        return self.ela

    def calc(self, samples, label="tmp"):
        from . import elasticity
        strucs = samples[0] if isinstance(samples, tuple) else samples
        if len(strucs) == 0:
            return np.zeros(0, dtype=float)
        if self.relaxer is not None:
            strucs, _ = self.relaxer(list(strucs), None)
        res = elasticity.analyze_records(self._analysis(), list(strucs))
        self.last = res
        status = np.asarray(res["status"])
        out = np.array(res[self.quantity][:, self.AVERAGES.index(self.average)], dtype=float)
        fine = status == 0
        if self.average == "voigt":
            fine |= status == 2   # SINGULAR keeps the Voigt values
        else:
            with np.errstate(invalid="ignore"):
                fine &= np.asarray(res["cond"]) <= self.cond_max
        if self.require_stable:
            fine &= np.asarray(res["n_negative"]) == 0
        out[~fine] = np.nan
        return out


class Symmetry:
    """A symmetry figure (symmetry.find_symmetry) as a calculator of `Reward.prop_cfg`: `.calc(samples, label)` returns
    `quantity` per structure -- n_ops (operations of the cell as given, pure translations included), pg_order (the point group's order),
    not_p1 (1.0 when there is any operation beyond the pure translations, else 0.0), crystal_system (1 triclinic .. 7 cubic), or, through
    symmetry.conventional_records, bravais (1 .. 14 in the order aP mP mS oP oS oI oF tP tI hR hP cP cI cF) or centring_mult
    (the lattice points per conventional cell: 1, 2, 3 or 4), or, through symmetry.refined_records, n_orbits (the
    symmetry-inequivalent sites of the cell as given) or distortion (the root mean square distance in A between the atoms and their
    places in the structure projected onto the group found).  NaN (->
    failed -> reward 0) on any status other than OK: a crystal the prepare guard flags, an ambiguous tolerance, more operations than the
    cap, a set that is not a group.  symprec in A (0.1: the reference's SpacegroupAnalyzer value)."""

    QUANTITIES = ("n_ops", "pg_order", "not_p1", "crystal_system", "bravais", "centring_mult", "n_orbits", "distortion")

    def __init__(self, quantity="n_ops", symprec=0.1, angle_tol=5.0, root_dir="rewards", device="cuda", **kwargs):
        if quantity not in self.QUANTITIES:
            raise ValueError(f"Symmetry: quantity {quantity!r} is none of {self.QUANTITIES}")
        if not (np.isfinite(symprec) and symprec > 0):
            raise ValueError(f"Symmetry: symprec = {symprec!r} is not a positive length")
        self.quantity, self.symprec, self.angle_tol, self.root_dir, self.device = quantity, float(symprec), float(angle_tol), root_dir, device

    def calc(self, samples, label="tmp"):
        from . import _lib, symmetry
        strucs = samples[0] if isinstance(samples, tuple) else samples
        if len(strucs) == 0:
            return np.zeros(0, dtype=float)
        if self.quantity in ("bravais", "centring_mult"):
            _, conv = symmetry.conventional_records(list(strucs), self.symprec, self.angle_tol, self.device)
            out = (conv.bravais_index if self.quantity == "bravais" else conv.mult).astype(float)
            out[conv.status != _lib.SYM_OK] = np.nan
            return out
        if self.quantity in ("n_orbits", "distortion"):
            _, ref = symmetry.refined_records(list(strucs), self.symprec, self.angle_tol, self.device)
            out = (ref.n_orbits if self.quantity == "n_orbits" else ref.rms_move).astype(float)
            out[ref.status != _lib.SYM_OK] = np.nan
            return out
        res = symmetry.find_symmetry(list(strucs), self.symprec, self.angle_tol, self.device)
        col = "pg_order" if self.quantity == "not_p1" else self.quantity
        out = getattr(res, col).astype(float)
        if self.quantity == "not_p1":
            out = (out > 1).astype(float)
        out[res.status != _lib.SYM_OK] = np.nan
        return out


class PyMatGen:
    """The composition / cell properties of rewards/calculators/pymatgen/calc.py:163-205 that need no external database:
    `density` (g/cm^3, :45-53).  `hhi` (:57-73) is the mass-fraction-weighted Herfindahl-Hirschman index of the elements'
    geological reserves; pymatgen ships that table as data (hhi.csv), which is not available offline -- pass `hhi_table`
    (CSV: symbol, HHI production, HHI reserve) to use it; without the table the task fails per sample (NaN -> reward 0, as the
    reference's calculators do on error, :84-89).  `mcia` (:115-160) is the minimal coincident interface area (A^2) between each
    structure and `substrate` on the device (matinvent_amd.substrates): `substrate` is a substrates.Substrate, a cell (six
    parameters or a 3 x 3 matrix) or a file structure.read_extxyz reads -- no table of named substrates is shipped; `substrate_millers`
    lists the substrate's planes (the reference uses (1, 0, 0) for Si, GaAs and InP), `zsl` holds substrates.ZSL arguments; NaN on any
    status other than OK, as the reference's `except` branch does.  conventional=True puts every film into its conventional cell first
    (symmetry.conventional_records), as the reference does before its substrate analysis (:136-160; its own cell conventions
    are [UPSTREAM-UNVERIFIED]); it excludes primitive=True.  `abundance` / `log_abundance` are the mass-fraction-weighted crustal abundance
    of the elements and its log10, from the `abundance` column of the user's element table (`element_table`: a chemistry.ElementTable or
    the path of its JSON file): NaN when an element's value is missing or the weighted value is not positive, as the reference's `abundance_crust` (:23-44).  `price` stays refused."""

    def __init__(self, root_dir="rewards", task="density", hhi_table=None, substrate=None, substrate_millers=None, zsl=None, primitive=False, device="cuda",
                 conventional=False, element_table=None, **kwargs):
        assert task in ("density", "hhi", "mcia", "abundance", "log_abundance"), f"task {task!r} needs pymatgen / SMACT data that this build does not carry"
        self.root_dir, self.task = root_dir, task
        self.hhi = None
        if task in ("abundance", "log_abundance"):
            from .chemistry import ElementTable
            if element_table is None:
                raise ValueError(f"task {task!r} needs element_table= (a chemistry.ElementTable or the path of its JSON file): no table is shipped")
            self.element_table = element_table if isinstance(element_table, ElementTable) else ElementTable.load(element_table)
        if task == "mcia":
            import os
            from . import substrates
            if substrate is None or isinstance(substrate, str) and not os.path.exists(substrate):
                raise ValueError(f"task 'mcia' needs substrate= as a Substrate, a cell or a file (got {substrate!r}): no table of named substrates is shipped")
            self.zsl = substrates.ZSL(**dict(zsl or {}))
            if isinstance(substrate, substrates.Substrate):
                if substrate_millers is not None:
                    raise ValueError("substrate_millers goes with a cell or a file: a Substrate carries its own planes")
                self.substrate = substrate
            else:
                self.substrate = substrates.Substrate("substrate", substrate, substrate_millers)
            if primitive and conventional:
                raise ValueError("task 'mcia': primitive=True and conventional=True exclude each other: the planes are indexed in one cell")
            self.primitive, self.conventional, self.device, self.bank = bool(primitive), bool(conventional), device, None
        if hhi_table is not None:
            import csv
            with open(hhi_table) as f:
                self.hhi = {r[0].strip(): float(r[2]) for r in csv.reader(f) if len(r) >= 3 and not r[0].startswith("#")}

    def calc(self, samples, label="tmp"):
        from .structure import MASSES, SYMBOLS, density
        strucs = samples[0] if isinstance(samples, tuple) else samples
        if self.task == "mcia":
            from . import substrates
            if self.bank is None:   # the tables are built once, at the first call
                self.bank = substrates.SubstrateBank([self.substrate], self.zsl, self.device)
            extra = dict(conventional=True) if self.conventional else {}   # (unset: the call as it was before the keyword)
            area, status = substrates.mcia(list(strucs), self.bank, self.zsl, primitive=self.primitive, device=self.device, **extra)
            return np.where(status == 0, area, np.nan).astype(float)
        out = []
        for s in strucs:
            try:
                if self.task == "density":
                    out.append(density(s.species, s.lengths, s.angles))
                elif self.task in ("abundance", "log_abundance"):
                    m = np.array([MASSES[int(z)] for z in s.species])
                    ab = np.array([self.element_table.abundance[int(z)] for z in s.species])
                    v = float((m / m.sum() * ab).sum())   # (an element without a value is NaN in the table)
                    if not v > 0.0:
                        raise ValueError("missing or non-positive abundance")
                    out.append(float(np.log10(v)) if self.task == "log_abundance" else v)
                else:
                    if self.hhi is None:
                        raise KeyError("no HHI table")
                    m = np.array([MASSES[int(z)] for z in s.species])
                    out.append(float(sum(mi / m.sum() * self.hhi[SYMBOLS[int(z)]] for mi, z in zip(m, s.species))))
            except Exception:
                out.append(np.nan)
        return np.array(out, dtype=float)
