"""Symmetry-constrained sampling (include/matinvent_hip_symc.h): `SymmetryConstraint` names, per crystal of a batch, a group
of operations g_k(f) = f W_k^-1 + t_k in the basis of the crystal's own cell, the orbits of the atoms under it and, per atom, the affine
map from its orbit representative's coordinates to its own.  DiffCSPModule.sample(..., symmetry=c) projects the state onto that group at
the start and after every reverse step: every state of the chain carries the template's group to float32 rounding, whatever the network
predicts.  Host bookkeeping only (pure numpy; nothing here needs a device but `template`, which runs the symmetry finder); the projection
is symmetry_project_kernel (csrc/sym_constraint.hip)."""
import ctypes as C
import json

import numpy as np
import torch

MAX_ATOMS, MAX_OPS = 256, 192   # include/matinvent_hip_symc.h


def refuse(where, **keys):
    """A projected state has no likelihood under the recorded proposal: sample_mdp / sample_rollout / MatInventPG refuse the symmetry keys."""
    for k, v in keys.items():
        if v is not None and v is not False:
            raise ValueError(f"{where}: {k} is not supported -- a symmetry-constrained chain projects every state, and a projected state has no "
                             "likelihood under the recorded proposal (DESIGN 57)")


def _centre(v):
    return v - np.round(v)


class _Part:
    """One crystal: n atoms, K operations W [K, 3, 3] int32 / t [K, 3], the site maps sigma [K, n], the operations `distinct` [R] whose
    rotation parts are the distinct ones, per atom the representative rep, the operation kof that carries the representative to the atom,
    Q [n, 9] and d [n, 3]; types [n] of the template, or None."""

    def __init__(self, n, W, t, sigma, distinct, rep, kof, Q, d, types=None):
        self.n, self.W, self.t, self.sigma, self.distinct = int(n), W, t, sigma, distinct
        self.rep, self.kof, self.Q, self.d, self.types = rep, kof, Q, d, types

    @property
    def K(self):
        return len(self.W)

    @classmethod
    def identity(cls, n, types=None):
        n = int(n)
        return cls(n, np.eye(3, dtype=np.int32).reshape(1, 3, 3), np.zeros((1, 3)), np.arange(n, dtype=np.int64).reshape(1, n), np.zeros(1, np.int32),
                   np.arange(n, dtype=np.int32), np.zeros(n, np.int32), np.tile(np.eye(3).reshape(1, 9), (n, 1)), np.zeros((n, 3)),
                   None if types is None else np.asarray(types, np.int64).reshape(n))


def _inverse_int(W, what):
    """The integer inverses of unimodular W [K, 3, 3]."""
    Wi = np.zeros_like(W)
    for k in range(len(W)):
        det = int(round(float(np.linalg.det(W[k].astype(np.float64)))))
        if det not in (1, -1):
            raise ValueError(f"{what}: det W = {det} for operation {k}: the rotation part of an operation is a lattice map (det +-1)")
        Wi[k] = np.round(np.linalg.inv(W[k].astype(np.float64))).astype(W.dtype)
        if not np.array_equal(Wi[k] @ W[k], np.eye(3, dtype=W.dtype)):
            raise ValueError(f"{what}: operation {k} has no integer inverse")
    return Wi


def _site_maps(frac, Wi, t, tol, types, what):
    """sigma [K, n]: the atom (of i's species, when types are given) nearest to g_k(x_i), the distance being the Euclidean length of the
    centred fractional difference; every map must land within tol and be a bijection."""
    K, n = len(Wi), len(frac)
    sigma = np.zeros((K, n), np.int64)
    same = None if types is None else (types[:, None] == types[None, :])
    for k in range(K):
        y = frac @ Wi[k].astype(np.float64) + t[k]
        dist = np.sqrt((_centre(y[:, None, :] - frac[None, :, :]) ** 2).sum(-1))
        if same is not None:
            dist = np.where(same, dist, np.inf)
        j = dist.argmin(1)
        worst = dist[np.arange(n), j].max() if n else 0.0
        if not worst <= tol:
            raise ValueError(f"{what}: broken site map -- operation {k} carries an atom {worst:.3g} (fractional) away from the nearest atom, tol = {tol:g}")
        if len(set(int(v) for v in j)) != n:
            raise ValueError(f"{what}: broken site map -- operation {k} does not permute the atoms")
        sigma[k] = j
    return sigma


def _closure(Wi, t, tol, what):
    """The multiplication table of the operations modulo lattice translations: m[k, l] with g_k o g_l = g_m, and the centred defects
    c[k, l] = t_l W_k^-1 + t_k - t_m.  ValueError: not a group."""
    K = len(Wi)
    key = lambda M: np.asarray(M, np.int64).tobytes()
    classes, cls_of = {}, np.zeros(K, np.int64)
    for k in range(K):
        cls_of[k] = classes.setdefault(key(Wi[k]), len(classes))
    R = len(classes)
    if K % R:
        raise ValueError(f"{what}: not a group -- {K} operations over {R} distinct rotation parts")
    Tn = K // R
    members = np.full((R, Tn), -1, np.int64)
    fill = np.zeros(R, np.int64)
    for k in range(K):
        c = cls_of[k]
        if fill[c] >= Tn:
            raise ValueError(f"{what}: not a group -- a rotation part occurs more often than the others")
        members[c, fill[c]] = k
        fill[c] += 1
    first = members[:, 0]
    if key(np.eye(3)) not in classes:
        raise ValueError(f"{what}: not a group -- the identity is missing")
    prod = np.zeros((R, R), np.int64)   # the class of W_l^-1 W_k^-1, by the classes of k and l
    for a in range(R):
        for b in range(R):
            c = classes.get(key(Wi[first[b]] @ Wi[first[a]]))
            if c is None:
                raise ValueError(f"{what}: not a group -- the product of two rotation parts is not among them")
            prod[a, b] = c
    tt = np.einsum("lj,kjc->klc", t, Wi.astype(np.float64)) + t[:, None, :]          # [k, l] = t_l W_k^-1 + t_k
    cand = members[prod[cls_of[:, None], cls_of[None, :]]]                           # [K, K, Tn]
    diff = _centre(tt[:, :, None, :] - t[cand])                                      # [K, K, Tn, 3]
    err = np.abs(diff).max(-1)
    pick = err.argmin(-1)
    kk, ll = np.meshgrid(np.arange(K), np.arange(K), indexing="ij")
    if not (err[kk, ll, pick] <= tol).all():
        raise ValueError(f"{what}: not a group -- a product of two operations is no operation of the list (translation off by "
                         f"{float(err[kk, ll, pick].max()):.3g}, tol = {tol:g})")
    m = cand[kk, ll, pick]
    if any(len(set(int(v) for v in m[k])) != K for k in range(K)):
        raise ValueError(f"{what}: not a group -- the same operation is listed twice")
    return m, diff[kk, ll, pick], [int(v) for v in first]


def _build_part(n, frac, W, t, tol, types, what):
    n = int(n)
    frac = np.asarray(frac, np.float64).reshape(-1, 3)
    W = np.asarray(W)
    if W.size == 0 or not np.array_equal(W, np.round(W)):
        raise ValueError(f"{what}: W must hold integers ([K, 3, 3], K >= 1)")
    W = np.round(W).astype(np.int32).reshape(-1, 3, 3)
    t = np.asarray(t, np.float64).reshape(-1, 3)
    K = len(W)
    if len(frac) != n or len(t) != K:
        raise ValueError(f"{what}: {len(frac)} coordinate rows for {n} atoms, {len(t)} translations for {K} rotation parts")
    if K > MAX_OPS:
        raise ValueError(f"{what}: {K} operations exceed the cap of {MAX_OPS}")
    if not (np.isfinite(frac).all() and np.isfinite(t).all()):
        raise ValueError(f"{what}: non-finite coordinates or translations")
    types = None if types is None else np.asarray(types, np.int64).reshape(n)
    if K == 1:
        if not np.array_equal(W[0], np.eye(3, dtype=np.int32)) or np.abs(_centre(t[0])).max() > tol:
            raise ValueError(f"{what}: not a group -- a single operation must be the identity")
        return _Part.identity(n, types)
    if n > MAX_ATOMS:
        raise ValueError(f"{what}: {n} atoms exceed the cap of {MAX_ATOMS}")
    Wi = _inverse_int(W, what)
    sigma = _site_maps(frac, Wi, t, tol, types, what)
    m, defect, distinct = _closure(Wi, t, tol, what)
    if not np.array_equal(sigma[m], sigma[:, sigma]):   # [k, l, i]: sigma_m(i) = sigma_k(sigma_l(i))
        raise ValueError(f"{what}: broken site map -- the maps of a product are not the product of the maps")
    # the translations with the closure defects averaged out: t_k - (sum_p c(k, p)) / K closes exactly where the input closes to tol
    t = t - defect.sum(1) / float(K)
    ident = int(np.where([np.array_equal(W[k], np.eye(3, dtype=np.int32)) and np.abs(_centre(t[k])).max() <= tol for k in range(K)])[0][0])
    rep = sigma.min(0).astype(np.int32)
    kof = np.zeros(n, np.int32)
    Q, d = np.zeros((n, 9)), np.zeros((n, 3))
    for r in sorted(set(int(v) for v in rep)):
        stab = [k for k in range(K) if sigma[k, r] == r]
        orbit = sorted(set(int(v) for v in sigma[:, r]))
        if len(orbit) * len(stab) != K:
            raise ValueError(f"{what}: not a group -- atom {r}: {len(orbit)} atoms in the orbit x site order {len(stab)} is not {K}")
        Ws = Wi[stab].astype(np.float64)
        shift = np.round(frac[r] - (frac[r] @ Ws + t[stab]))              # n_k: g_k + n_k fixes the template position
        P, c = Ws.mean(0), (t[stab] + shift).mean(0)
        for j in orbit:
            k = ident if j == r else int(np.where(sigma[:, r] == j)[0][0])
            kof[j] = k
            Q[j] = (P @ Wi[k].astype(np.float64)).reshape(9)
            d[j] = c @ Wi[k].astype(np.float64) + t[k]
    return _Part(n, W, t, sigma, np.asarray(distinct, np.int32), rep, kof, Q, d, types)


class SymmetryConstraint:
    """The symmetry constraint of B crystals with N atoms in all (one _Part per crystal).  It has `.num_atoms`, so it can stand in as the
    `batch` argument of DiffCSPModule.sample; `.atom_types` [N] are the template's (None when a crystal has none)."""

    def __init__(self, parts):
        self.parts = list(parts)
        self.num_atoms = torch.tensor([p.n for p in self.parts], dtype=torch.long)

    def __len__(self):
        return len(self.parts)

    @property
    def num_nodes(self):
        return int(self.num_atoms.sum())

    @property
    def num_ops(self):
        return [p.K for p in self.parts]

    @property
    def atom_types(self):
        if any(p.types is None for p in self.parts):
            return None
        return torch.as_tensor(np.concatenate([p.types for p in self.parts]) if self.parts else np.zeros(0, np.int64), dtype=torch.long)

    @property
    def orbit(self):
        """[N] the orbit representative of every atom, an index inside its crystal."""
        return np.concatenate([p.rep for p in self.parts]) if self.parts else np.zeros(0, np.int32)

    def operations(self, i):
        """(W [K, 3, 3] int32, t [K, 3], sigma [K, n]) of crystal i: g_k(f) = f W_k^-1 + t_k carries atom j onto atom sigma[k, j]."""
        p = self.parts[i]
        return p.W, p.t, p.sigma

    # ---- constructors --------------------------------------------------------------------------------
    @classmethod
    def from_operations(cls, num_atoms, frac, W, t, tol=1e-3, atom_types=None, copies=1):
        """`copies` crystals of `num_atoms` atoms at the template positions frac [n, 3] under the operations (W [K, 3, 3] integers, t
        [K, 3]) given in the template's own basis.  tol: the largest fractional distance between the image of an atom and the atom it is
        mapped onto, and between a product's translation and the listed one.  atom_types [n]: maps stay inside a species.  ValueError by
        name: a list that is not a group, a broken site map, more than 192 operations or (with more than the identity) 256 atoms."""
        part = _build_part(num_atoms, frac, W, t, float(tol), atom_types, "SymmetryConstraint.from_operations")
        return cls([part] * int(copies))

    @classmethod
    def identity(cls, num_atoms, atom_types=None):
        """The identity alone for crystals of these atom counts: free crystals, to be stacked beside constrained ones."""
        na = [int(v) for v in np.asarray(num_atoms).reshape(-1)]
        off = np.concatenate([[0], np.cumsum(na)])
        return cls([_Part.identity(n, None if atom_types is None else np.asarray(atom_types)[off[i]:off[i + 1]]) for i, n in enumerate(na)])

    @classmethod
    def template(cls, record, copies, symprec=0.1, angle_tol=5.0, device="cuda", tol=1e-3):
        """`copies` crystals with the space group and the orbits of `record` (SimpleStructure / CrystalData-like): the record refined onto the
        group found at symprec (refined_records, cell="given"), analysed again, the operations carried from the reduced basis of the
        prepared set into the record's own.  ValueError by name: a template whose analysis is not OK."""
        from . import _lib, matching
        from . import symmetry as S
        refined, res = S.refined_records([record], symprec, angle_tol, device, cell="given")
        if int(res.info[0, 7]) != _lib.SYM_OK:
            raise ValueError(f"SymmetryConstraint.template: the template's refinement has status {int(res.info[0, 7])}, not OK")
        na, offsets, types, frac, lat, tols = S._upload(refined, device, symprec)
        prepared = matching.prepare_arrays(offsets, types, frac, lat)
        sym = S.find_symmetry_prepared(prepared, tols, angle_tol)
        if int(sym.status[0]) != _lib.SYM_OK:
            raise ValueError(f"SymmetryConstraint.template: the refined template's analysis has status {int(sym.status[0])}, not OK")
        Wr, tr, _ = sym.operations(0)
        n = int(na[0])
        L = lat[0].reshape(3, 3).double().cpu().numpy()
        Lr = prepared.lat[0].reshape(3, 3).double().cpu().numpy()
        scale = (float(n) / abs(float(np.linalg.det(L)))) ** (1.0 / 3.0)
        Tf = Lr @ np.linalg.inv(L) / scale                      # the prepared set's transform: (scaled) reduced cell = T x cell
        T = np.round(Tf).astype(np.int64)
        if np.abs(Tf - T).max() > 1e-4 or int(round(float(np.linalg.det(T)))) not in (1, -1):
            raise ValueError("SymmetryConstraint.template: the prepared set's transform could not be recovered")
        Ti = np.round(np.linalg.inv(T.astype(np.float64))).astype(np.int64)
        W = np.stack([Ti @ Wr[k].astype(np.int64) @ T for k in range(len(Wr))])      # f = f_r T: W^-1 = T^-1 W_r^-1 T
        t = np.asarray(tr, np.float64) @ T.astype(np.float64)
        part = _build_part(n, frac.double().cpu().numpy(), W, t, float(tol), types.cpu().numpy(), "SymmetryConstraint.template")
        return cls([part] * int(copies))

    def slice(self, g0, g1):
        """The constraint of the contiguous crystal group g0 .. g1 - 1."""
        return SymmetryConstraint(self.parts[int(g0):int(g1)])

    def select(self, idx):
        """The constraint of the crystals `idx`, in that order."""
        return SymmetryConstraint([self.parts[int(i)] for i in idx])

    @staticmethod
    def stack(constraints):
        """The constraints of several crystal groups as one, in that order (mixed batches: SymmetryConstraint.identity for the free crystals)."""
        return SymmetryConstraint([p for c in constraints for p in c.parts])

    def condition(self, types=True):
        """The conditioning.Condition that fixes every atom type to the template's (types: a bool or a per-atom mask over all N atoms)."""
        from .conditioning import Condition
        at = self.atom_types
        if at is None:
            raise ValueError("SymmetryConstraint.condition: the constraint holds no template atom types")
        N = self.num_nodes
        known = torch.full((N,), bool(types), dtype=torch.bool) if isinstance(types, (bool, np.bool_)) else torch.as_tensor(np.asarray(types)).bool().flatten()
        cond = Condition(self.num_atoms, atom_types=at, known_types=known)
        self.check_condition(cond)
        return cond

    def check_condition(self, cond, where="SymmetryConstraint"):
        """What a condition beside this constraint must be (ValueError): for the same crystals, on atom types alone, and the atoms of every
        orbit share their known type."""
        if [int(v) for v in cond.num_atoms.tolist()] != [int(v) for v in self.num_atoms.tolist()]:
            raise ValueError(f"{where}: the condition's atom counts are not the symmetry constraint's")
        if bool(cond.known_coords.any()) or bool(cond.known_lattice.any()):
            raise ValueError(f"{where}: a condition that knows a coordinate or a lattice does not go with a symmetry constraint -- only atom types")
        kt, z = cond.known_types.numpy(), cond.atom_types.numpy()
        n0 = 0
        for g, p in enumerate(self.parts):
            r = n0 + p.rep.astype(np.int64)
            sl = slice(n0, n0 + p.n)
            if (kt[sl] != kt[r]).any() or (kt[sl] & (z[sl] != z[r])).any():
                raise ValueError(f"{where}: crystal {g}: the atoms of an orbit do not share their known type")
            n0 += p.n

    # ---- the handle ----------------------------------------------------------------------------------
    def arrays(self):
        """The flat host arrays of mi_symmetry_constraint: op_off [B + 1], rot [sum K, 9], distinct_off [B + 1], distinct, rep [N], Q [N, 9], d [N, 3]."""
        P = self.parts
        i32 = lambda v: np.ascontiguousarray(np.asarray(v).astype(np.int32))
        cat = lambda vs, shape, dt: np.ascontiguousarray(np.concatenate(vs).astype(dt)) if vs else np.zeros(shape, dt)
        return dict(op_off=i32(np.concatenate([[0], np.cumsum([p.K for p in P])])), rot=cat([p.W.reshape(-1, 9) for p in P], (0, 9), np.int32),
                    distinct_off=i32(np.concatenate([[0], np.cumsum([len(p.distinct) for p in P])])), distinct=cat([p.distinct for p in P], (0,), np.int32),
                    rep=cat([p.rep for p in P], (0,), np.int32), Q=cat([p.Q for p in P], (0, 9), np.float64), d=cat([p.d for p in P], (0, 3), np.float64))

    def attach(self, cb):
        """Copy this constraint to the batch handle `cb` (mi_batch_set_symmetry: blocking copies; no work of the handle may be in flight)."""
        from . import _lib
        if cb.num_atoms_list != [int(v) for v in self.num_atoms.tolist()]:
            raise ValueError("SymmetryConstraint: its atom counts are not those of the batch it is attached to")
        a = self.arrays()
        st = _lib.SymmetryConstraint(*(a[k].ctypes.data for k in ("op_off", "rot", "distinct_off", "distinct", "rep", "Q", "d")))
        _lib.check(_lib.load().mi_batch_set_symmetry(cb._h, C.byref(st)), "mi_batch_set_symmetry")

    @staticmethod
    def clear(cb):
        from . import _lib
        _lib.check(_lib.load().mi_batch_set_symmetry(cb._h, None), "mi_batch_set_symmetry")


stack = SymmetryConstraint.stack


def apply(cb, atom_types, frac_coords, lattices):
    """mi_symmetry_apply: impose the constraint attached to `cb` on a state (device tensors, float32, contiguous; in place), on the current stream."""
    from . import _lib
    from .cspnet import _ptr, _stream
    for v in (atom_types, frac_coords, lattices):
        assert v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()
    assert atom_types.shape[0] == cb.num_nodes and frac_coords.shape[0] == cb.num_nodes and lattices.shape[0] == cb.num_graphs
    _lib.check(_lib.load().mi_symmetry_apply(cb._h, _ptr(atom_types), _ptr(frac_coords), _ptr(lattices), _stream()), "mi_symmetry_apply")


def failures(cb):
    """mi_symmetry_failures: [B] the crystals' counts of skipped cell projections since the last call (cleared).  Drains the device first."""
    from . import _lib
    torch.cuda.synchronize()
    out = np.zeros(max(cb.num_graphs, 1), np.int32)
    _lib.check(_lib.load().mi_symmetry_failures(cb._h, out.ctypes.data_as(C.POINTER(C.c_int))), "mi_symmetry_failures")
    return out[:cb.num_graphs].astype(np.int64)


def load_template(path):
    """A template record from a JSON file {lengths: [3], angles: [3] (degrees), species: [n] atomic numbers, frac_coords: [n][3]}."""
    from .data import SimpleStructure
    with open(path) as f:
        d = json.load(f)
    missing = [k for k in ("lengths", "angles", "species", "frac_coords") if k not in d]
    if missing:
        raise ValueError(f"symmetry template {path}: missing {missing}")
    return SimpleStructure([float(v) for v in d["lengths"]], [float(v) for v in d["angles"]], [int(v) for v in d["species"]],
                           np.asarray(d["frac_coords"], np.float64).reshape(-1, 3))
