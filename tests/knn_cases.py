"""Shared inputs of the large knn tests (tests/test_gpu_knn_large.py): fixed seeds, built on the CPU, each oracle result computed once.

Two kinds of geometry:
  dense(na)   cell lengths 3.5 .. 9 A, angles 65 .. 115 deg, fractional coordinates uniform in [0, 1): about twenty kept neighbours per
              atom, the max-neighbour trim active (what tests/test_gpu_knn.py::_random_crystals draws);
  sparse(na)  lattices = N(0, 1) entries -- what a reverse chain starts from: skewed, left-handed and near-singular cells, a cutoff
              of a fraction of an Angstrom and a handful of edges -- with coordinates uniform in [-1, 2), outside the home cell.

The edge list is compared bit for bit, so no candidate pair may sit on a decision boundary of the reference's float32 arithmetic:
`margin` recomputes every candidate's d^2 in float64 and returns the smallest relative distance to a boundary.  The seeds below were
chosen so that it exceeds MARGIN_MIN (tests/test_knn_cases.py checks that without a GPU, and every GPU test asserts it again before it
compares): a bit mismatch then cannot be blamed on a borderline input.
"""
import functools

import numpy as np
import torch

from oracle import diffcsp_oracle as O

MAX_NEIGHBORS = 20
MARGIN_MIN = 1e-5

# atoms per crystal
BATCH_A = [20] * 52 + [13]            # 1 053 atoms: the scan kernel's chunk is 2 over the atoms; 96 N = 101 088 capacity rows: the striding Fourier launch
BATCH_B = [1, 2, 3] * 350             # 2 100 atoms in 1 050 crystals: chunk 3 over the atoms, chunk 2 over the crystals
BATCH_C = [64, 64] + [1] * 1100       # the 64-atom limit beside a scan over more than 1 024 entries of either table
BATCH_G = [20] * 24 + [13, 1, 7]      # 501 atoms, about 10 k edges: above the 8 192 from which the backward forms dZ2 as a plane set

CASES = {   # name -> (atoms per crystal, kind, seed)
    "A_dense": (BATCH_A, "dense", 471),
    "A_sparse": (BATCH_A, "sparse", 102),
    "B_dense": (BATCH_B, "dense", 113),
    "B_sparse": (BATCH_B, "sparse", 104),
    "C_dense": (BATCH_C, "dense", 195),
    "G_dense": (BATCH_G, "dense", 146),
}


def dense(num_atoms, seed, lo=3.5, hi=9.0, ang=(65.0, 115.0)):
    g = torch.Generator().manual_seed(seed)
    B, N = len(num_atoms), sum(num_atoms)
    lengths = lo + (hi - lo) * torch.rand(B, 3, generator=g)
    angles = ang[0] + (ang[1] - ang[0]) * torch.rand(B, 3, generator=g)
    lat = O.lattice_params_to_matrix(lengths, angles)
    frac = torch.rand(N, 3, generator=g)
    return frac, lat


def sparse(num_atoms, seed):
    g = torch.Generator().manual_seed(seed)
    B, N = len(num_atoms), sum(num_atoms)
    lat = torch.randn(B, 3, 3, generator=g)
    frac = 3.0 * torch.rand(N, 3, generator=g) - 1.0
    return frac, lat


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(frac [N,3], lattices [B,3,3], num_atoms [B]) of a named case; the same tensors on every call -- do not modify them."""
    na, kind, seed = CASES[name]
    frac, lat = (dense if kind == "dense" else sparse)(na, seed)
    return frac, lat, torch.tensor(na)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(edges [2,E], edge_vec [E,3]) of a named case from the oracle, in the reference's order; computed once."""
    frac, lat, na = inputs(name)
    return O.knn_edges(frac, lat, na, MAX_NEIGHBORS)


def margin(frac, lattices, num_atoms, max_neighbors=MAX_NEIGHBORS):
    """Smallest relative distance of any candidate pair's d^2 (float64, from the float32 inputs) to a decision boundary of
    radius_graph_pbc: cutoff^2 = (smallest inter-plane spacing + 0.01)^2, the self-pair floor 1e-4, and -- for a centre with more than
    `max_neighbors` candidates inside the cutoff -- the trim threshold d^2_(max_neighbors) + 0.01.  Relative to the boundary's value: the
    float32 evaluation of d^2 (three products of differences of O(cell) terms) is good to a few 1e-7 of the larger of the two."""
    frac, L = frac.double().numpy(), lattices.double().numpy()
    cells = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], dtype=np.float64)
    best, off = np.inf, 0
    for b, n in enumerate(int(v) for v in num_atoms):
        Lb = L[b]
        vol = np.dot(Lb[0], np.cross(Lb[1], Lb[2]))
        spacing = [1.0 / np.linalg.norm(np.cross(Lb[(k + 1) % 3], Lb[(k + 2) % 3]) / vol) for k in range(3)]
        r2 = (min(spacing) + 0.01) ** 2
        cart = frac[off:off + n] @ Lb                                             # [n,3]
        d = cart[:, None, None, :] - (cart[None, :, None, :] + (cells @ Lb)[None, None, :, :])
        d2 = (d ** 2).sum(-1).reshape(n, n * 27)                                  # [centre, candidate]
        rel = lambda x, bound: np.abs(x - bound) / bound
        best = min(best, float(rel(d2, r2).min()), float(rel(d2, 1e-4).min()))
        inside = (d2 <= r2) & (d2 > 1e-4)
        for i in range(n):
            di = np.sort(d2[i][inside[i]])
            if max_neighbors > 0 and di.size > max_neighbors:
                best = min(best, float(rel(di, di[max_neighbors] + 0.01).min()))
        off += n
    return best


@functools.lru_cache(maxsize=None)
def case_margin(name):
    frac, lat, na = inputs(name)
    return margin(frac, lat, na)


def max_degree(edges, num_nodes):
    """Largest degree in a symmetric list.  An atom's degree bounds the neighbours it keeps as a centre, so a list whose largest degree
    is at most edge_cap_per_node is inside every capacity of a handle (kept neighbours <= cap, degree <= 2 cap, edges <= 2 cap N)."""
    return int(torch.bincount(edges[0], minlength=num_nodes).max()) if edges.numel() else 0
