"""DiffCSPSampler: host glue around DiffCSPModule.sample (models/diffcsp/sample.py:117-201)."""
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from .data import CrystalData, data2struc, lattices_to_params_shape

# atom-count prior of MP-20 (data table, sample.py:42-62) and the generation step size (:82)
ATOM_DIST = {"mp_20": [0.0, 0.0021742334905660377, 0.021079009433962265, 0.019826061320754717, 0.15271226415094338,
                       0.047132959905660375, 0.08464770047169812, 0.021079009433962265, 0.07808814858490566,
                       0.03434551886792453, 0.0972877358490566, 0.013303360849056603, 0.09669811320754718,
                       0.02155807783018868, 0.06522700471698113, 0.014372051886792452, 0.06703272405660378,
                       0.00972877358490566, 0.053176591981132074, 0.010576356132075472, 0.08995430424528301]}
DEFAULT_STEP_LR = {"gen": {"perov_5": 1e-6, "carbon_24": 1e-5, "mp_20": 5e-6}}


class SampleDataset:
    """sample.py:117-138: draws num_atoms from the numpy GLOBAL generator, like the reference."""

    def __init__(self, total_num, dataset="mp_20"):
        self.total_num = total_num
        self.distribution = ATOM_DIST[dataset]
        self.num_atoms = np.random.choice(len(self.distribution), total_num, p=self.distribution)

    def __len__(self):
        return self.total_num


class _AtomCounts:
    def __init__(self, num_atoms):
        self.num_atoms = torch.as_tensor(np.asarray(num_atoms), dtype=torch.long)


@dataclass
class DiffCSPSampler:
    batch_size: Optional[int] = None
    num_batches: Optional[int] = None
    target_compositions_dict: Optional[list] = None
    num_atoms_distribution: str = "mp_20"
    seed: int = 0

    def generate(self, model, batch_size=None, num_batches=None, sample_steps=None, condition=None, target_compositions_dict=None,
                 resample_times=None, jump_length=None, properties_to_condition_on=None, diffusion_guidance_factor=None, steer=None,
                 classifier=None, symmetry_template=None, symmetry_fix_types=False, **kwargs) -> Tuple[List[CrystalData], list]:
        """sample.py:148-201.  Extra kwargs (`max_num`, `filter`, ...) are tolerated like the reference.
        `sample_steps` = S: the chains run on S of the model's T trained steps (model.respaced(S)); None: all of them.
        As in the reference, every batch is sampled but only the LAST batch's outputs are unpacked
        (sample.py:166-177).  `rank`/`world_size` kwargs shard the batch by crystal (DP): each rank
        samples a contiguous block with global noise offsets and the records are all-gathered.

        Conditioned generation (DiffCSPModule.sample's `condition`): `target_compositions_dict` -- this keyword, else the
        field -- is a list of {symbol: count} mappings; the batch_size x num_batches crystals cycle through it, every atom type is
        fixed (Condition.composition) and the atom counts come from the compositions instead of the mp_20 draw.  `condition`: an explicit
        conditioning.Condition for all batch_size x num_batches crystals, or for batch_size of them (then used for every batch).
        `resample_times` = r with `jump_length` = j (DiffCSPModule.sample's `resample`): the conditioned chains make RePaint's
        resampling jumps; both or neither, and only with a condition (ValueError).  Levels are step indices under `sample_steps`.
        `properties_to_condition_on` = {name: value} with `diffusion_guidance_factor` = gamma (default 0; DiffCSPModule.sample's
        `guidance`): every crystal is sampled under these property values by a property-conditioned model, with classifier-free guidance
        of that factor.  ValueError: a factor without properties, either together with a condition.
        `steer` (DiffCSPModule.sample's `steer`): a steering.Steering, or the mapping of sample_cfg.steer (Steering.from_config).
        The batch_size crystals become the groups: every drawn atom count is replicated K times and G K records come back; the events'
        ancestors and statistics of the last batch are left in `self.last_steer`.  ValueError: together with a condition, resampling,
        guidance, or more than one rank.
        `classifier` (DiffCSPModule.sample's `classifier`): a classifier.ClassifierGuidance, or the mapping of
        sample_cfg.classifier (ClassifierGuidance.from_config).  The guided steps and the predictor's outputs along the last batch's chain
        are left in `self.last_classifier`.  ValueError: together with steer, a condition, resampling, guidance, or more than one rank.
        `symmetry_template` (DiffCSPModule.sample's `symmetry`): a crystal record, or the path of a JSON file holding one
        (symmetry_constraint.load_template); every one of the batch_size x num_batches crystals is sampled under the template's space group
        and Wyckoff multiplicities (SymmetryConstraint.template), with the template's atom count.  `symmetry_fix_types`: its species are
        fixed too, by a condition on the atom types.  The cell-projection failure counts of the last batch are left in
        `self.last_symmetry`.  ValueError: together with a condition, resampling, guidance, steer or classifier."""
        batch_size = batch_size or self.batch_size
        num_batches = num_batches or self.num_batches
        assert batch_size is not None and num_batches is not None
        targets = target_compositions_dict if target_compositions_dict is not None else self.target_compositions_dict
        if targets is not None and len(targets) == 0:
            targets = None
        if targets is not None:
            if condition is not None:
                raise ValueError("DiffCSPSampler.generate: give target_compositions_dict or condition, not both")
            from .conditioning import Condition
            condition = Condition.composition(list(targets), batch_size * num_batches)
        elif condition is not None and len(condition) not in (batch_size, batch_size * num_batches):
            raise ValueError(f"DiffCSPSampler.generate: the condition covers {len(condition)} crystals, not batch_size = {batch_size} or "
                             f"batch_size x num_batches = {batch_size * num_batches}")
        if (resample_times is None) != (jump_length is None):
            raise ValueError("DiffCSPSampler.generate: give resample_times and jump_length together, or neither")
        resample = None if resample_times is None else (resample_times, jump_length)
        if resample is not None and condition is None:
            raise ValueError("DiffCSPSampler.generate: resample_times / jump_length need a condition (target_compositions_dict or condition)")
        guide = None
        if properties_to_condition_on:
            if condition is not None:
                raise ValueError("DiffCSPSampler.generate: properties_to_condition_on together with a condition is not supported")
            from .guidance import Guidance
            guide = Guidance({k: float(v) for k, v in dict(properties_to_condition_on).items()}, diffusion_guidance_factor or 0.0)
        elif diffusion_guidance_factor:
            raise ValueError("DiffCSPSampler.generate: diffusion_guidance_factor needs properties_to_condition_on")
        constraint = None
        if symmetry_template is not None:
            from .symmetry_constraint import SymmetryConstraint, load_template
            for name, v in (("a condition", condition is not None), ("resample_times", resample is not None), ("properties_to_condition_on", guide is not None),
                            ("steer", steer is not None), ("classifier", classifier is not None)):
                if v:
                    raise ValueError(f"DiffCSPSampler.generate: symmetry_template together with {name} is not supported")
            record = load_template(symmetry_template) if isinstance(symmetry_template, (str, bytes)) or hasattr(symmetry_template, "__fspath__") else symmetry_template
            constraint = SymmetryConstraint.template(record, batch_size, device=getattr(model, "device", "cuda"))
            if symmetry_fix_types:
                condition = constraint.condition(types=True)
        elif symmetry_fix_types:
            raise ValueError("DiffCSPSampler.generate: symmetry_fix_types needs symmetry_template")
        rank, world = int(kwargs.get("rank", 0)), int(kwargs.get("world_size", 1))
        if steer is not None:
            from .steering import Steering
            for name, v in (("a condition", condition is not None), ("resample_times", resample is not None),
                            ("properties_to_condition_on", guide is not None), (f"world_size = {world}", world > 1)):
                if v:
                    raise ValueError(f"DiffCSPSampler.generate: steer together with {name} is not supported")
            steer = Steering.from_config(steer, device=getattr(model, "device", None))
        if classifier is not None:
            from .classifier import ClassifierGuidance
            for name, v in (("steer", steer is not None), ("a condition", condition is not None), ("resample_times", resample is not None),
                            ("properties_to_condition_on", guide is not None), (f"world_size = {world}", world > 1)):
                if v:
                    raise ValueError(f"DiffCSPSampler.generate: classifier together with {name} is not supported")
            classifier = ClassifierGuidance.from_config(classifier, device=getattr(model, "device", None))
        model = _strided(model, sample_steps)
        model.eval()
        from .dist import collectives_on
        if constraint is not None:   # the atom counts are the template's
            from types import SimpleNamespace
            dataset = SimpleNamespace(num_atoms=np.tile(constraint.num_atoms.numpy(), num_batches))
        elif condition is not None:   # the atom counts are the condition's: nothing is drawn, so every rank holds the same vector
            from types import SimpleNamespace
            dataset = SimpleNamespace(num_atoms=np.tile(condition.num_atoms.numpy(), batch_size * num_batches // len(condition)))
        else:
            dataset = SampleDataset(total_num=batch_size * num_batches, dataset=self.num_atoms_distribution)
        if condition is None and constraint is None and (world > 1 or collectives_on()):
            # the atom counts come from numpy's unseeded GLOBAL generator (sample.py:123): every rank would draw a different
            # vector, while the shard ranges and the global noise offsets below assume ONE.  Rank 0's draw is the batch.
            from .dist import broadcast_object
            dataset.num_atoms = np.asarray(broadcast_object(dataset.num_atoms.tolist(), src=0))
        step_lr = DEFAULT_STEP_LR["gen"]["mp_20"]
        outputs = None
        for bi in range(num_batches):
            na = dataset.num_atoms[bi * batch_size:(bi + 1) * batch_size]
            from .dist import shard_range
            lo, hi = shard_range(len(na), rank, world)
            node_off = int(np.sum(na[:lo]))
            self.seed += 1
            counts = _AtomCounts(na[lo:hi] if steer is None else np.asarray(steer.replicate(na[lo:hi])))
            if steer is not None:
                outputs, _, self.last_steer = model.sample(counts, step_lr=step_lr, seed=self.seed, node_offset=node_off, graph_offset=lo, steer=steer)
                continue
            if classifier is not None:
                outputs, _, self.last_classifier = model.sample(counts, step_lr=step_lr, seed=self.seed, node_offset=node_off, graph_offset=lo,
                                                                classifier=classifier)
                continue
            cond = None
            if condition is not None:
                c0 = bi * batch_size % len(condition)
                cond = condition.slice(c0 + lo, c0 + hi)
            if constraint is not None:
                outputs, _, self.last_symmetry = model.sample(counts, step_lr=step_lr, seed=self.seed, node_offset=node_off, graph_offset=lo, condition=cond,
                                                              symmetry=constraint.slice(lo, hi))
                continue
            outputs, _ = model.sample(counts, step_lr=step_lr, seed=self.seed, node_offset=node_off, graph_offset=lo, condition=cond,
                                      **({} if resample is None else {"resample": resample}), **({} if guide is None else {"guidance": guide}))
        data_list = _unpack(model, counts, outputs, node_off, lo, where="DiffCSPSampler.generate")
        struc_list = [data2struc(d) for d in data_list]
        if world > 1 or collectives_on():
            from .dist import all_gather_objects
            parts = all_gather_objects((data_list, struc_list))
            data_list = [d for p in parts for d in p[0]]
            struc_list = [s for p in parts for s in p[1]]
        return data_list, struc_list


def _unpack(model, counts, outputs, node_offset=0, graph_offset=0, where="sample_loop / sample_mdp"):
    """The final state of a `model.sample` call as CrystalData records (sample.py:178-195, :221-244), each carrying the device-side geometry
    that invalid_filter thresholds (K18), computed where the state lives.  node_offset / graph_offset: the shard's position in its batch
    (DiffCSPSampler.generate under DP); `where` labels a saturation error."""
    from . import _lib
    from .structure import check_structures
    if hasattr(model, "check_graph"):
        model.check_graph()   # (knn edge style: the chains' neighbour lists stayed inside their capacity -- the device is about to be drained anyway)
    _lib.check_saturation(where)  # (the results are about to be copied to the host: the device is drained anyway)
    geom = check_structures(model.crystal_batch(counts, node_offset, graph_offset), outputs["frac_coords"], outputs["lattices"]).cpu()
    frac_coords = outputs["frac_coords"].detach().cpu()
    num_atoms = outputs["num_atoms"].detach().cpu()
    atom_types = torch.argmax(outputs["atom_types"].detach().cpu(), dim=-1) + 1  # sample.py:182
    lengths, angles = lattices_to_params_shape(outputs["lattices"].detach().cpu())
    offset = [0] + torch.cumsum(num_atoms, dim=0).tolist()
    data_list = []
    for i in range(len(num_atoms)):
        d = CrystalData(frac_coords=frac_coords[offset[i]:offset[i + 1]], atom_types=atom_types[offset[i]:offset[i + 1]],
                        lengths=lengths[i].view(1, -1), angles=angles[i].view(1, -1), num_atoms=int(num_atoms[i]))
        d.geometry = {"max_cell_edge": float(geom[i, 0]), "min_distance": float(geom[i, 1]), "volume": float(geom[i, 2])}
        data_list.append(d)
    return data_list


def _draw_seed(seed):
    # the reference's noise comes from torch's global generator: so does the Philox key here, unless the caller names one
    return int(torch.randint(0, 2 ** 62, (1,))) if seed is None else int(seed)


def _strided(model, sample_steps):
    """`model`, or with sample_steps = S its view on S of its T steps (DiffCSPModule.respaced; S = T is the model itself)."""
    if sample_steps is None:
        return model
    if not hasattr(model, "respaced"):
        raise ValueError(f"sample_steps = {sample_steps}: {type(model).__name__} has no strided reverse chain")
    return model.respaced(int(sample_steps))


def _prelude(sample_size, model, step_lr):
    """What sample_loop / sample_mdp / sample_rollout do before model.sample: eval mode, the atom-count draw (numpy's global generator) and
    the step_lr default.  Returns (counts, step_lr); the callers draw their seed (_draw_seed) after it, as before."""
    model.eval()
    dataset = SampleDataset(total_num=sample_size)
    return _AtomCounts(dataset.num_atoms), (step_lr if step_lr >= 0 else DEFAULT_STEP_LR["gen"]["mp_20"])


def sample_loop(sample_size, model, device=None, step_lr=-1, seed=None):
    """sample.py:204-246: one batch of `sample_size` crystals (atom counts from the MP-20 prior) -> list of CrystalData."""
    counts, step_lr = _prelude(sample_size, model, step_lr)
    outputs, _ = model.sample(counts, step_lr=step_lr, seed=_draw_seed(seed))
    return _unpack(model, counts, outputs)


def _refuse_condition(where, condition):
    if condition is not None:
        raise ValueError(f"{where}: a condition is not supported -- a conditioned chain's recorded log-probabilities are those of the "
                         "unconditioned proposal, not a trajectory likelihood (DESIGN 31)")


def sample_mdp(sample_size, model, device=None, step_lr=-1, seed=None, sample_steps=None, condition=None, resample=None, steer=None, classifier=None,
               symmetry=None, smact=None):
    """sample.py:249-309: sample with the trajectory recorded and return (sample_list, sample_traj), restricted to the crystals that
    pass invalid_filter.  sample_traj[k] is the step t = T - k (t = T .. 2) with the reference's keys (atom_types, lattices, frac_coords,
    frac_coords_mid, num_atoms, timesteps, log_prob_{t,x,l}; host tensors) plus next_frac_coords / next_lattices / next_atom_types --
    the state at t - 1 -- so that any element can go straight to DiffCSPModule.forward_logprb.  (The reference's own sample_mdp unpacks
    invalid_filter into the wrong values and never builds the next_* keys that forward_logprb reads.)
    A strided view (DiffCSPModule.respaced), or sample_steps = S which builds it: T is the view's S and `timesteps` are step indices --
    what the VIEW's forward_logprb takes.  A `condition` is refused (ValueError), and so are `resample` and `symmetry`.
    smact: a chemistry.SmactValidity, handed to invalid_filter."""
    from .filters import invalid_filter
    from .resampling import refuse
    refuse("sample_mdp", resample=resample)
    from .steering import refuse as refuse_steer
    refuse_steer("sample_mdp", steer=steer)   # (a resampled particle system has no per-chain trajectory likelihood)
    from .classifier import refuse as refuse_classifier
    refuse_classifier("sample_mdp", classifier=classifier)   # (the record would be the unshifted proposal's)
    from .symmetry_constraint import refuse as refuse_symmetry
    refuse_symmetry("sample_mdp", symmetry=symmetry)   # (a projected state has no likelihood under the recorded proposal)
    from .guidance import refuse_latent
    refuse_latent(model, "sample_mdp")
    _refuse_condition("sample_mdp", condition)
    model = _strided(model, sample_steps)
    counts, step_lr = _prelude(sample_size, model, step_lr)
    outputs, traj = model.sample(counts, step_lr=step_lr, seed=_draw_seed(seed), record=True)
    data_list = _unpack(model, counts, outputs)
    valid = invalid_filter(data_list, return_mask=True, **({} if smact is None else {"smact": smact}))
    sample_list = [d for d, ok in zip(data_list, valid) if ok]
    valid_idx = torch.as_tensor(np.where(valid)[0], dtype=torch.long)
    atom_bool = torch.as_tensor(valid)[traj[0]["batch_idx"].cpu()]
    cpu = lambda v: v.detach().cpu()
    sample_traj = []
    for i in range(model.beta_scheduler.timesteps, 1, -1):
        cur, nxt = traj[i], traj[i - 1]
        gi = valid_idx.to(cur["lattices"].device)
        ai = atom_bool.to(cur["atom_types"].device)
        sample_traj.append({
            "atom_types": cpu(cur["atom_types"][ai]),
            "lattices": cpu(cur["lattices"][gi]),
            "frac_coords": cpu(cur["frac_coords"][ai]),
            "frac_coords_mid": cpu(cur["frac_coords_mid"][ai]),
            "num_atoms": cpu(cur["num_atoms"][gi]),
            "timesteps": torch.tensor([i] * len(valid_idx), dtype=torch.long),
            "log_prob_t": cpu(cur["log_prob_t"][gi]),
            "log_prob_x": cpu(cur["log_prob_x"][gi]),
            "log_prob_l": cpu(cur["log_prob_l"][gi]),
            "next_frac_coords": cpu(nxt["frac_coords"][ai]),
            "next_lattices": cpu(nxt["lattices"][gi]),
            "next_atom_types": cpu(nxt["atom_types"][ai]),
        })
    return sample_list, sample_traj


@dataclass
class Rollout:
    """The kept crystals' reverse-diffusion chains on the device, stacked over t = 0..T (index t = the state at diffusion time t):
    atom_types [T+1, N, 100], frac_coords / frac_coords_mid [T+1, N, 3], lattices [T+1, B, 9], lp_old [T+1, B, 3] = the sampler's own
    recorded (log_prob_l, log_prob_t, log_prob_x) of the step t -> t-1 (defined for t = 2..T).  num_atoms: host long [B]; node_offsets:
    host long [B+1]; step_lr: the step size the chain ran with (mi_traj_pg_step re-evaluates with the same one).  condition: None, or
    the conditioning.Condition of the kept crystals when the chain was sampled with likelihood="free" -- lp_old is then the masked record
    and policy.pg_step re-evaluates under the same masks."""
    atom_types: torch.Tensor
    frac_coords: torch.Tensor
    frac_coords_mid: torch.Tensor
    lattices: torch.Tensor
    lp_old: torch.Tensor
    num_atoms: torch.Tensor
    node_offsets: torch.Tensor
    T: int
    step_lr: float
    condition: Optional[object] = None

    @property
    def num_graphs(self):
        return len(self.num_atoms)

    def select(self, idx):
        """The rollout restricted to crystals `idx` (in that order): one compaction per array."""
        idx = [int(i) for i in idx]
        if idx == list(range(self.num_graphs)):
            return self
        gi = torch.as_tensor(idx, dtype=torch.long)
        ai = torch.cat([torch.arange(int(self.node_offsets[i]), int(self.node_offsets[i + 1])) for i in idx]) if idx else torch.zeros(0, dtype=torch.long)
        dev = self.atom_types.device
        gd, ad = gi.to(dev), ai.to(dev)
        na = self.num_atoms[gi]
        return Rollout(self.atom_types.index_select(1, ad), self.frac_coords.index_select(1, ad), self.frac_coords_mid.index_select(1, ad),
                       self.lattices.index_select(1, gd), self.lp_old.index_select(1, gd), na,
                       torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(na, 0)]), self.T, self.step_lr,
                       None if self.condition is None else self.condition.select(idx))


def sample_rollout(sample_size, model, step_lr=-1, seed=None, geometric_filter=True, sample_steps=None, condition=None, likelihood=None,
                   resample=None, steer=None, classifier=None, symmetry=None, smact=None):
    """Sample like sample_mdp (same atom-count draw, seed handling and invalid_filter; geometric_filter=False keeps every crystal) and
    keep the kept crystals' whole trajectories on the device as a Rollout -- compacted once per chain straight from the sampler's stacked
    record buffers, without the per-step dict or a host copy.  Returns (sample_list, rollout).  The policy gradient (policy.pg_step)
    consumes it.  CSP mode (keep_lattice / keep_coords) is refused: forward_logprb does not model it.
    A strided view (DiffCSPModule.respaced), or sample_steps = S which builds it: rollout.T = S, the arrays are [S + 1, ...] and index k is
    the state at step index k (trained time tau_k); pg_step then takes the same view as its agent.  A `condition` alone is refused
    (ValueError), like CSP mode.
    condition=c (for `sample_size` crystals), likelihood="free" (DESIGN 36): the chains are conditioned on c, whose atom counts replace the
    draw; rollout.lp_old is the masked record (the predictor terms of the known elements left out) and rollout.condition the kept
    crystals' part of c, which pg_step re-evaluates under.  CSP mode stays refused.  `resample` is refused (ValueError): a resampled chain
    visits levels more than once and a rollout holds one visit.  `symmetry` is refused too.
    smact: a chemistry.SmactValidity, handed to invalid_filter; with geometric_filter=False its mask alone decides."""
    from .conditioning import check_likelihood
    from .filters import invalid_filter
    from .resampling import refuse
    refuse("sample_rollout", resample=resample)
    from .steering import refuse as refuse_steer
    refuse_steer("sample_rollout", steer=steer)   # 
    from .classifier import refuse as refuse_classifier
    refuse_classifier("sample_rollout", classifier=classifier)   # 
    from .symmetry_constraint import refuse as refuse_symmetry
    refuse_symmetry("sample_rollout", symmetry=symmetry)   # 
    from .guidance import refuse_latent
    refuse_latent(model, "sample_rollout")
    if not check_likelihood("sample_rollout", likelihood, condition):
        _refuse_condition("sample_rollout", condition)
    elif len(condition) != int(sample_size):
        raise ValueError(f"sample_rollout: the condition covers {len(condition)} crystals, sample_size is {sample_size}")
    model = _strided(model, sample_steps)
    if getattr(model, "keep_lattice", False) or getattr(model, "keep_coords", False):
        raise ValueError("sample_rollout: CSP mode (keep_lattice / keep_coords) is not supported -- forward_logprb does not model a given "
                         "lattice or given coordinates")
    counts, step_lr = _prelude(sample_size, model, step_lr)
    if condition is not None:   # (the atom counts are the condition's; the draw above is made all the same, so the global generator moves as without one)
        counts = _AtomCounts(condition.num_atoms)
    sink = []
    outputs, _ = model.sample(counts, step_lr=step_lr, seed=_draw_seed(seed), record=True, rec_sink=sink, condition=condition, likelihood=likelihood)
    data_list = _unpack(model, counts, outputs)
    if smact is None:
        valid = invalid_filter(data_list, return_mask=True) if geometric_filter else np.ones(len(data_list), dtype=bool)
    else:
        valid = invalid_filter(data_list, return_mask=True, smact=smact) if geometric_filter else np.asarray(smact(data_list), dtype=bool)
    sample_list = [d for d, ok in zip(data_list, valid) if ok]
    valid = torch.as_tensor(np.asarray(valid, dtype=bool))
    na = counts.num_atoms
    T = model.beta_scheduler.timesteps
    sink.sort(key=lambda e: e[0])
    bounds = [e[0] for e in sink] + [len(na)]
    parts = {k: [] for k in ("atom_types", "frac_coords", "frac_coords_mid", "lattices", "lp_old")}
    for k, (g0, n0, rec) in enumerate(sink):
        g1 = bounds[k + 1]
        gv = valid[g0:g1]
        dev = rec["lattices"].device
        gi = torch.nonzero(gv).flatten().to(dev)
        ai = torch.nonzero(torch.repeat_interleave(gv, na[g0:g1])).flatten().to(dev)
        parts["atom_types"].append(rec["atom_types"].index_select(1, ai))
        parts["frac_coords"].append(rec["frac_coords"].index_select(1, ai))
        parts["frac_coords_mid"].append(rec["frac_coords_mid"].index_select(1, ai))
        parts["lattices"].append(rec["lattices"].view(T + 1, -1, 9).index_select(1, gi))
        parts["lp_old"].append(torch.stack((rec["log_prob_l"], rec["log_prob_t"], rec["log_prob_x"]), dim=-1).index_select(1, gi))
    st = {k: (v[0] if len(v) == 1 else torch.cat(v, dim=1)) for k, v in parts.items()}
    kept = na[valid]
    rollout = Rollout(st["atom_types"], st["frac_coords"], st["frac_coords_mid"], st["lattices"], st["lp_old"], kept,
                      torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(kept, 0)]), T, float(step_lr),
                      None if condition is None else condition.select(torch.nonzero(valid).flatten().tolist()))
    return sample_list, rollout
