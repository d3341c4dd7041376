"""Replacement conditioning of the reverse chain (include/matinvent_hip_cond.h): `Condition` names the part of a batch of
crystals that is known -- atom types and fractional coordinates per atom, the lattice per crystal -- and holds its clean values.
DiffCSPModule.sample(..., condition=c) overwrites that part, after every reverse step, with a forward-noised copy of the clean value at
the level the chain has reached (RePaint, Lugmayr et al. 2022): the network always sees inputs at the noise level it was trained for,
and at level 0 the known part is exact.  Host bookkeeping only; the imposition is condition_impose_kernel (csrc/condition.hip)."""
import ctypes as C
import re

import numpy as np
import torch

from .structure import SYMBOLS

_Z = {s: z for z, s in enumerate(SYMBOLS) if z > 0}
_TOKEN = re.compile(r"([A-Z][a-z]?)(\d*)")


def parse_composition(spec) -> dict:
    """{symbol: count} of a mapping (`{"Li": 2, "O": 1}`, as in target_compositions_dict) or a formula string ("Li2O")."""
    if isinstance(spec, str):
        text = spec.replace(" ", "")
        tokens = _TOKEN.findall(text)
        if not tokens or "".join(s + n for s, n in tokens) != text:
            raise ValueError(f"cannot parse the formula {spec!r}")
        pairs = [(s, int(n) if n else 1) for s, n in tokens]
    else:
        pairs = [(str(s), v) for s, v in dict(spec).items()]
    out = {}
    for s, n in pairs:
        if s not in _Z:
            raise ValueError(f"unknown element {s!r} (the model knows Z = 1..100)")
        if int(n) != n or int(n) < 0:
            raise ValueError(f"{s}: the atom count must be a non-negative integer (got {n!r})")
        if int(n):
            out[s] = out.get(s, 0) + int(n)
    if not out:
        raise ValueError(f"empty composition {spec!r}")
    return out


def composition_types(spec) -> list:
    """The atomic numbers of one crystal of that composition, ordered by atomic number."""
    return sorted(z for s, n in parse_composition(spec).items() for z in [_Z[s]] * n)


def level_table(module) -> torch.Tensor:
    """[T + 1, 3] float32 (sqrt(abar_k), sqrt(1 - abar_k), sigma_k) from the module's own schedulers, computed as add_noise computes them
    (diffcsp.py: torch.sqrt of the float32 table).  On a strided view these are the view's tables: level k is its step index."""
    ac = module.beta_scheduler.alphas_cumprod.detach().cpu().float()
    sig = module.sigma_scheduler.sigmas.detach().cpu().float()
    return torch.stack([torch.sqrt(ac), torch.sqrt(1.0 - ac), sig], dim=1).contiguous()


def _mask(v, counts, what):
    """bool / per-atom mask of ONE crystal -> per-atom bool tensor."""
    if isinstance(v, (bool, np.bool_)):
        return torch.full((counts,), bool(v), dtype=torch.bool)
    m = torch.as_tensor(np.asarray(v)).bool().flatten()
    if len(m) != counts:
        raise ValueError(f"{what}: a per-atom mask needs {counts} entries (got {len(m)})")
    return m


class Condition:
    """The known part of B crystals with N atoms in all.

    num_atoms [B]; atom_types [N] (atomic numbers 1..100) with known_types [N]; frac_coords [N, 3] with known_coords [N] (an atom's
    three coordinates together); lattices [B, 3, 3] -- or lengths + angles (degrees), converted like CSP mode's -- with known_lattice
    [B].  A mask left out means "none known"; values where a mask is False are never read.  Host tensors.  It has `.num_atoms`, so it
    can stand in as the `batch` argument of DiffCSPModule.sample."""

    def __init__(self, num_atoms, atom_types=None, known_types=None, frac_coords=None, known_coords=None, lattices=None, lengths=None,
                 angles=None, known_lattice=None):
        self.num_atoms = torch.as_tensor(np.asarray(num_atoms)).long().flatten()
        B, N = len(self.num_atoms), int(self.num_atoms.sum())
        host = lambda v, dt: torch.as_tensor(np.asarray(v.detach().cpu()) if torch.is_tensor(v) else np.asarray(v)).to(dt)
        self.atom_types = torch.ones(N, dtype=torch.long) if atom_types is None else host(atom_types, torch.long).flatten()
        self.known_types = torch.zeros(N, dtype=torch.bool) if known_types is None else host(known_types, torch.bool).flatten()
        self.frac_coords = torch.zeros(N, 3) if frac_coords is None else host(frac_coords, torch.float32).reshape(-1, 3)
        self.known_coords = torch.zeros(N, dtype=torch.bool) if known_coords is None else host(known_coords, torch.bool).flatten()
        if lattices is None and lengths is not None:
            from .data import lattice_params_to_matrix
            lattices = lattice_params_to_matrix(host(lengths, torch.float32).reshape(-1, 3), host(angles, torch.float32).reshape(-1, 3))
        self.lattices = torch.zeros(B, 3, 3) if lattices is None else host(lattices, torch.float32).reshape(-1, 3, 3)
        self.known_lattice = torch.zeros(B, dtype=torch.bool) if known_lattice is None else host(known_lattice, torch.bool).flatten()
        for name, n in (("atom_types", N), ("known_types", N), ("frac_coords", N), ("known_coords", N), ("lattices", B), ("known_lattice", B)):
            if len(getattr(self, name)) != n:
                raise ValueError(f"Condition: {name} has {len(getattr(self, name))} rows, the atom counts give {n}")
        kt = self.atom_types[self.known_types]
        if len(kt) and (int(kt.min()) < 1 or int(kt.max()) > 100):
            raise ValueError("Condition: a known atom type lies outside 1..100")
        if (int(self.known_types.sum()) and atom_types is None) or (int(self.known_coords.sum()) and frac_coords is None) or \
                (int(self.known_lattice.sum()) and lattices is None):
            raise ValueError("Condition: a mask marks elements as known whose clean values were not given")

    def __len__(self):
        return len(self.num_atoms)

    @property
    def num_nodes(self):
        return int(self.num_atoms.sum())

    # ---- constructors --------------------------------------------------------------------------------
    @classmethod
    def composition(cls, counts_or_formula, copies):
        """`copies` crystals whose every atom type is fixed and nothing else: a mapping {symbol: count}, a formula string, or a list of
        either (like target_compositions_dict) that the crystals cycle through.  Atoms are ordered by atomic number."""
        specs = list(counts_or_formula) if isinstance(counts_or_formula, (list, tuple)) else [counts_or_formula]
        if not specs:
            raise ValueError("Condition.composition: no composition given")
        per = [composition_types(s) for s in specs]
        zs = [per[i % len(per)] for i in range(int(copies))]
        types = torch.tensor([z for c in zs for z in c], dtype=torch.long)
        return cls([len(c) for c in zs], atom_types=types, known_types=torch.ones(len(types), dtype=torch.bool))

    @classmethod
    def template(cls, crystal, copies, types=True, coords=False, lattice=False):
        """`copies` crystals shaped like `crystal` (frac_coords [n, 3], atom_types [n], lengths / angles [1, 3] or `lattices` [3, 3]: a
        CrystalData, for one) with the chosen parts known.  types / coords: a bool or a per-atom mask; lattice: a bool."""
        copies = int(copies)
        n = int(np.asarray(crystal.atom_types).shape[0])
        mt, mx = _mask(types, n, "types"), _mask(coords, n, "coords")
        ml = bool(np.asarray(lattice).all()) if not isinstance(lattice, bool) else lattice
        rep = lambda v, dt: torch.as_tensor(np.asarray(v)).to(dt)
        kw = {}
        if getattr(crystal, "lattices", None) is not None:
            kw["lattices"] = rep(crystal.lattices, torch.float32).reshape(1, 3, 3).repeat(copies, 1, 1)
        else:
            kw["lengths"] = rep(crystal.lengths, torch.float32).reshape(1, 3).repeat(copies, 1)
            kw["angles"] = rep(crystal.angles, torch.float32).reshape(1, 3).repeat(copies, 1)
        return cls([n] * copies, atom_types=rep(crystal.atom_types, torch.long).flatten().repeat(copies), known_types=mt.repeat(copies),
                   frac_coords=rep(crystal.frac_coords, torch.float32).reshape(n, 3).repeat(copies, 1), known_coords=mx.repeat(copies),
                   known_lattice=torch.full((copies,), ml, dtype=torch.bool), **kw)

    def slice(self, g0, g1):
        """The condition of the contiguous crystal group g0 .. g1 - 1."""
        off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(self.num_atoms, 0)])
        a0, a1 = int(off[g0]), int(off[g1])
        return Condition(self.num_atoms[g0:g1], atom_types=self.atom_types[a0:a1], known_types=self.known_types[a0:a1],
                         frac_coords=self.frac_coords[a0:a1], known_coords=self.known_coords[a0:a1], lattices=self.lattices[g0:g1],
                         known_lattice=self.known_lattice[g0:g1])

    def select(self, idx):
        """The condition of the crystals `idx`, in that order (any subset: the kept crystals of a filtered rollout)."""
        idx = [int(i) for i in idx]
        off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(self.num_atoms, 0)])
        gi = torch.as_tensor(idx, dtype=torch.long)
        ai = torch.cat([torch.arange(int(off[i]), int(off[i + 1])) for i in idx]) if idx else torch.zeros(0, dtype=torch.long)
        return Condition(self.num_atoms[gi], atom_types=self.atom_types[ai], known_types=self.known_types[ai], frac_coords=self.frac_coords[ai],
                         known_coords=self.known_coords[ai], lattices=self.lattices[gi], known_lattice=self.known_lattice[gi])

    # ---- the handle ----------------------------------------------------------------------------------
    def attach(self, module, cb, table=None):
        """Copy this condition and `module`'s level table to the batch handle `cb` (mi_batch_set_condition: blocking copies; no work of
        the handle may be in flight).  `table`: a [n, 3] table instead of the module's (tests)."""
        from . import _lib
        if cb.num_atoms_list != [int(v) for v in self.num_atoms.tolist()]:
            raise ValueError("Condition: its atom counts are not those of the batch it is attached to")
        tab = (level_table(module) if table is None else torch.as_tensor(table).float()).contiguous().numpy()
        i32 = lambda v: np.ascontiguousarray(v.numpy().astype(np.int32))
        keep = [i32(self.known_types), i32(self.known_coords), i32(self.known_lattice), i32(self.atom_types),
                np.ascontiguousarray(self.frac_coords.numpy(), dtype=np.float32), np.ascontiguousarray(self.lattices.numpy(), dtype=np.float32)]
        st = _lib.Condition(*(a.ctypes.data for a in keep))
        _lib.check(_lib.load().mi_batch_set_condition(cb._h, C.byref(st), tab.ctypes.data_as(C.POINTER(C.c_float)), int(tab.shape[0])),
                   "mi_batch_set_condition")

    @staticmethod
    def clear(cb):
        from . import _lib
        _lib.check(_lib.load().mi_batch_set_condition(cb._h, None, None, 0), "mi_batch_set_condition")


    # ---- the likelihood mask (include/matinvent_hip_lik.h) -----------------------------------
    def attach_likelihood(self, module, cb):
        """Copy this condition's three masks to the batch handle `cb` as its likelihood mask (mi_batch_set_likelihood_mask: blocking
        copies; no work of the handle may be in flight): the predictor terms of the known elements leave the log-probabilities that
        mi_traj_logprob / mi_traj_pg_step / mi_traj_pg_kl_step compute on the handle and, with the condition attached too, the ones a
        recording chain records.  `module` is the handle's module, as for `attach` (the mask itself needs nothing of it)."""
        from . import _lib
        if cb.num_atoms_list != [int(v) for v in self.num_atoms.tolist()]:
            raise ValueError("Condition: its atom counts are not those of the batch it is attached to")
        i32 = lambda v: np.ascontiguousarray(v.numpy().astype(np.int32))
        keep = [i32(self.known_types), i32(self.known_coords), i32(self.known_lattice)]
        _lib.check(_lib.load().mi_batch_set_likelihood_mask(cb._h, *(a.ctypes.data_as(C.POINTER(C.c_int)) for a in keep)),
                   "mi_batch_set_likelihood_mask")

    @staticmethod
    def clear_likelihood(cb):
        from . import _lib
        _lib.check(_lib.load().mi_batch_set_likelihood_mask(cb._h, None, None, None), "mi_batch_set_likelihood_mask")


def check_likelihood(where, likelihood, condition):
    """The `likelihood` keyword of sample / sample_rollout / forward_logprb: None (the default) or "free" -- the trajectory likelihood
    over the free elements, which needs the condition that names them."""
    if likelihood not in (None, "free"):
        raise ValueError(f"{where}: likelihood = {likelihood!r} is neither None nor 'free'")
    if likelihood is not None and condition is None:
        raise ValueError(f"{where}: likelihood = 'free' needs the condition that names the free elements (condition=None)")
    return likelihood is not None


def apply(cb, level, seed, atom_types, frac_coords, lattices):
    """mi_condition_apply: impose the condition attached to `cb` on a state (device tensors, float32, contiguous; in place) at `level`,
    on the current stream."""
    from . import _lib
    from .cspnet import _ptr, _stream
    for v in (atom_types, frac_coords, lattices):
        assert v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()
    _lib.check(_lib.load().mi_condition_apply(cb._h, int(level), int(seed), _ptr(atom_types), _ptr(frac_coords), _ptr(lattices), _stream()),
               "mi_condition_apply")
