"""The RL loop's two memories, CPU bookkeeping around one device kernel.

`ReplayBuffer`: experience replay with the reference's surface and semantics (memory/replay_buffer.py:11-104): the rows of the
buffer and of the new samples are merged, de-duplicated on the composition's reduced formula keeping the highest reward (:78-91),
sorted by reward, cut to `buffer_size`, and THEN only rows with reward > reward_cutoff stay (:72-75); `sample` draws
min(len, sample_size) rows without replacement (:93-101); `memory_purge` drops the rows whose reduced formula is in the given
structures (:103-105).

`LongTimeMem`: every scored crystal so far and the diversity filter on it (memory/ltm.py:8-169), exact in the reference's two methods
("composition": reduced formula, "element_comb": sorted tuple of element symbols).

Beyond the reference, both take a STRUCTURE key: the pair (reduced formula, fingerprint cluster), where two crystals of one
formula are the same structure when their fingerprints (`structure.fingerprints`, a HIP kernel) lie within `fp_tol` in cosine distance.
A fixed-formula RL loop (sample_cfg.target_compositions_dict) has one reduced formula throughout: the composition key collapses the replay
buffer to one row and lets the diversity filter zero every reward; the structure key keeps `buffer_size` distinct structures."""
import csv

import numpy as np

from .structure import FP_TOL, SYMBOLS, cif_text, fingerprint_distance, record_fingerprints, reduced_formula


def _species(s):
    return [int(z) for z in (s.species if hasattr(s, "species") else np.asarray(s.atom_types).reshape(-1).tolist())]


def _formula(data):
    return reduced_formula(_species(data))


def _fingerprints_of(records, fingerprints, fp_args):
    """(fp, status) for `records`: the injected pair (tests, or a caller that has them already), else one device call."""
    if fingerprints is None:
        fingerprints = record_fingerprints(records, **(fp_args or {}))
    fp, status = fingerprints
    fp, status = np.asarray(fp, np.float32), np.asarray(status).astype(np.int64).reshape(-1)
    assert len(fp) == len(status) == len(records), "one fingerprint row and one status per record"
    return fp, status


class ReplayBuffer:
    def __init__(self, buffer_size=100, sample_size=8, reward_cutoff=0.0, seed=0, key="composition", fp_tol=FP_TOL, fp_args=None, **kwargs):
        if key not in ("composition", "structure"):
            raise ValueError(f"ReplayBuffer: key = {key!r} is neither 'composition' nor 'structure'")
        self.buffer_size, self.sample_size, self.reward_cutoff = buffer_size, sample_size, reward_cutoff
        self.key, self.fp_tol, self.fp_args = key, float(fp_tol), dict(fp_args or {})
        self.rows = []  # (reward, reduced formula, data[, fingerprint or None]), sorted by descending reward
        self.rng = np.random.default_rng(seed)

    def __len__(self):
        return len(self.rows)

    def _same(self, fa, pa, fb, pb):
        """The structure relation: one formula and fingerprints within fp_tol; a flagged crystal (no fingerprint) by formula alone, among
        the flagged."""
        if fa != fb or (pa is None) != (pb is None):
            return False
        return pa is None or float(fingerprint_distance(pa, pb)) <= self.fp_tol

    def extend(self, data_list, strucs, rewards, fingerprints=None):
        if self.key == "structure":
            fp, status = _fingerprints_of(data_list, fingerprints, self.fp_args)
            rows = self.rows + [(float(r), _formula(d), d, fp[i].copy() if status[i] == 0 else None) for i, (d, r) in enumerate(zip(data_list, rewards))]
            rows.sort(key=lambda x: -x[0])
            uniq = []
            for row in rows:                               # leader clustering in reward order: the first of a structure = its highest reward
                if not any(self._same(row[1], row[3], u[1], u[3]) for u in uniq):
                    uniq.append(row)
            self.rows = [row for row in uniq[: self.buffer_size] if row[0] > self.reward_cutoff]
            return
        rows = self.rows + [(float(r), _formula(d), d) for d, r in zip(data_list, rewards)]
        rows.sort(key=lambda x: -x[0])                     # stable: ties keep buffer-before-new order, like sort_values + concat
        seen, uniq = set(), []
        for row in rows:                                   # drop_duplicates(subset=["comp"]) keeps the first = highest reward
            if row[1] not in seen:
                seen.add(row[1])
                uniq.append(row)
        self.rows = [row for row in uniq[: self.buffer_size] if row[0] > self.reward_cutoff]

    def sample(self):
        if not self.rows:
            return [], np.zeros(0)
        idx = self.rng.choice(len(self.rows), size=min(self.sample_size, len(self.rows)), replace=False)
        return [self.rows[i][2] for i in idx], np.array([self.rows[i][0] for i in idx])

    def memory_purge(self, strucs, fingerprints=None):
        if self.key == "structure":
            if len(strucs) == 0 or not self.rows:
                return
            fp, status = _fingerprints_of(strucs, fingerprints, self.fp_args)
            gone = [(_formula(s), fp[i] if status[i] == 0 else None) for i, s in enumerate(strucs)]
            self.rows = [row for row in self.rows if not any(self._same(row[1], row[3], f, p) for f, p in gone)]
            return
        drop = set()
        for s in strucs:
            drop.add(reduced_formula(_species(s)))
        self.rows = [row for row in self.rows if row[1] not in drop]


class LongTimeMem:
    """memory/ltm.py: all scored crystals and their rewards; `div_filter` scales a reward down once its key has been seen more than `tol`
    times and zeroes it from `buff` on.  structure=True additionally assigns every row a (formula, fingerprint cluster) key as it comes in:
    within a formula, a crystal joins the first cluster whose representative (its founder) lies within fp_tol, else founds one; a flagged
    crystal (no fingerprint) is keyed by its formula alone.  One fp32 row per cluster is kept, none per crystal."""
    COLUMNS = ("struc", "comp", "ele_comb", "reward", "RL_step")

    def __init__(self, structure=False, fp_tol=FP_TOL, fp_args=None):
        self.memory = []            # rows: dict(struc, comp, ele_comb, reward, RL_step[, cluster])
        self.unique_comps = []      # reduced formulas in order of first appearance
        self.structure, self.fp_tol, self.fp_args = bool(structure), float(fp_tol), dict(fp_args or {})
        self._counts = {"comp": {}, "ele_comb": {}, "cluster": {}}
        self._reps = {}             # formula -> [fingerprint row of cluster 0, of cluster 1, ...]
        self._cluster_of = {}       # id(struc) -> cluster key of a stored row (the rows keep their structures alive)

    def __len__(self):
        return len(self.memory)

    @property
    def unique_structures(self):
        return len(self._counts["cluster"])

    @staticmethod
    def _keys(s):
        sp = _species(s)
        return reduced_formula(sp), tuple(sorted(set(SYMBOLS[z] for z in sp)))

    def _find(self, comp, fp, found):
        """The cluster key of a fingerprint within `comp`: the first representative within fp_tol; a new cluster when `found`, else None."""
        reps = self._reps.setdefault(comp, []) if found else self._reps.get(comp, [])
        for k, rep in enumerate(reps):
            if float(fingerprint_distance(rep, fp)) <= self.fp_tol:
                return (comp, k)
        if not found:
            return None
        reps.append(np.array(fp, np.float32))
        return (comp, len(reps) - 1)

    def extend(self, strucs, rewards, step, fingerprints=None):
        if self.structure:
            fp, status = _fingerprints_of(strucs, fingerprints, self.fp_args)
        for i, (s, r) in enumerate(zip(strucs, rewards)):
            comp, comb = self._keys(s)
            row = dict(struc=s, comp=comp, ele_comb=comb, reward=float(r), RL_step=step)
            if self.structure:
                row["cluster"] = self._find(comp, fp[i], True) if status[i] == 0 else (comp, -1)
                self._cluster_of[id(s)] = row["cluster"]
            for k in self._counts:
                if k in row:
                    self._counts[k][row[k]] = self._counts[k].get(row[k], 0) + 1
            if self._counts["comp"][comp] == 1:
                self.unique_comps.append(comp)
            self.memory.append(row)

    def div_filter(self, strucs, rewards, tol=10, buff=20, method="composition", fingerprints=None, **kwargs):
        """(new_rewards, penalty_idx, tol_n, buff_n), ltm.py:65-109; ref: Augmented Hill-Climb, doi 10.1186/s13321-022-00646-z.  The
        pipeline extends the memory before it filters, so a batch's own members count."""
        assert tol < buff
        if method == "composition":
            key, values = "comp", [self._keys(s)[0] for s in strucs]
        elif method == "element_comb":
            key, values = "ele_comb", [self._keys(s)[1] for s in strucs]
        elif method == "structure":
            if not self.structure:
                raise ValueError("div_filter(method='structure') needs LongTimeMem(structure=True): the clusters are assigned as rows come in")
            if "fp_tol" in kwargs and float(kwargs["fp_tol"]) != self.fp_tol:
                raise ValueError(f"div_filter: fp_tol = {kwargs['fp_tol']} differs from the {self.fp_tol} the memory clusters with")
            key, values = "cluster", [self._cluster_of.get(id(s)) for s in strucs]
            unknown = [i for i, v in enumerate(values) if v is None]           # crystals that were never stored: looked up, not added
            if unknown:
                fp, status = _fingerprints_of([strucs[i] for i in unknown], None if fingerprints is None else
                                              (np.asarray(fingerprints[0])[unknown], np.asarray(fingerprints[1])[unknown]), self.fp_args)
                for k, i in enumerate(unknown):
                    comp = self._keys(strucs[i])[0]
                    values[i] = self._find(comp, fp[k], False) if status[k] == 0 else (comp, -1)
        else:
            raise ValueError(f"div_filter: method = {method!r} is none of 'composition', 'element_comb', 'structure'")
        new_rewards, penalty_idx, tol_n, buff_n = [], [], 0, 0
        for i, v in enumerate(values):
            occ = self._counts[key].get(v, 0)
            if occ <= tol:
                new_rewards.append(rewards[i])
            elif occ > tol and occ < buff:
                new_rewards.append(rewards[i] * (buff - occ) / (buff - tol))
                tol_n += 1
            else:
                new_rewards.append(0.0)
                penalty_idx.append(i)
                buff_n += 1
        return np.array(new_rewards), penalty_idx, tol_n, buff_n

    def calc_metrics(self, thred, budget=3000, num_candidate=100):
        """(burden, div_ratio), ltm.py:111-134: scored crystals per unique composition whose best reward beats `thred` (None below
        `num_candidate` of them); unique compositions per scored crystal (None past `budget`)."""
        best = {}
        for row in self.memory:
            best[row["comp"]] = max(best.get(row["comp"], -np.inf), row["reward"])
        candidates = sum(1 for v in best.values() if v > thred)
        cost = len(self.memory)
        burden = cost / candidates if candidates >= num_candidate else None
        div_ratio = len(self.unique_comps) / cost if cost <= budget else None
        return burden, div_ratio

    def get_baseline(self, step, prev=3):
        r = [row["reward"] for row in self.memory if row["RL_step"] > step - prev]
        return float(np.mean(r)) if r else float("nan")

    def save(self, save_path):
        """The reference's columns plus `cif`, every field quoted (DataFrame.to_csv(index=False, quoting=1))."""
        with open(save_path, "w", newline="") as f:
            w = csv.writer(f, quoting=csv.QUOTE_ALL)
            w.writerow(list(self.COLUMNS) + ["cif"])
            for row in self.memory:
                w.writerow([f"{row['comp']} ({len(_species(row['struc']))} sites)"] + [row[k] for k in self.COLUMNS[1:]] + [cif_text(row["struc"])])
