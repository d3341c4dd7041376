"""Float64 restatement of replacement conditioning (matinvent_amd/csrc/condition.hip: condition_impose_kernel) with no device
code in it: the three imposition formulas of add_noise (diffusion.py:90-113)

    l = c0_k l0 + c1_k z        x = (x0 + sigma_k z) mod 1        a = c0_k onehot(type0) + c1_k z

applied to the KNOWN elements of a state only, the explicit level-0 branch (exactly l0, x0 mod 1, a 1.0 / 0.0 one-hot; no draw, the table
is not read), and the draws of the noise contract: oracle.diffcsp_oracle's numpy Philox with the draw ids 21 / 22 / 23, the step field =
the level and the element index (node_offset + atom) * width + column (graph_offset + crystal for the lattice).  Plain torch / numpy on
the CPU; shared by the CPU and the GPU tests.  `impose(..., dtype=torch.float32)` is the same formulas separately rounded in float32: the
yardstick of the device's tolerance."""
import numpy as np
import torch

from oracle import diffcsp_oracle as O

NUM_TYPES = 100
DRAW_COND_L, DRAW_COND_X, DRAW_COND_T = 21, 22, 23


def draws(seed, level, num_atoms, node_offset=0, graph_offset=0):
    """(z_l [B,3,3], z_x [N,3], z_t [N,100]) float32: the contract's normals of one imposition at `level` for a batch that starts at
    global atom `node_offset`, global crystal `graph_offset`."""
    na = torch.as_tensor(num_atoms).long()
    B, N = len(na), int(na.sum())
    f = lambda draw, n, off, *shape: torch.from_numpy(O.philox_normal(int(seed), int(level), draw, n, off).copy()).view(*shape)
    return (f(DRAW_COND_L, B * 9, graph_offset * 9, B, 3, 3), f(DRAW_COND_X, N * 3, node_offset * 3, N, 3),
            f(DRAW_COND_T, N * NUM_TYPES, node_offset * NUM_TYPES, N, NUM_TYPES))


def level_table(tables, dtype=torch.float64):
    """[T + 1, 3] = (sqrt(abar_k), sqrt(1 - abar_k), sigma_k) from dict(alphas_cumprod, sigmas), taken to `dtype` first."""
    ac, sig = tables["alphas_cumprod"].to(dtype), tables["sigmas"].to(dtype)
    return torch.stack([torch.sqrt(ac), torch.sqrt(1.0 - ac), sig], dim=1)


def impose(state, cond, table, level, z, dtype=torch.float64):
    """state = (atom_types [N,100], frac [N,3], lattices [B,3,3]); cond: anything with known_types / known_coords [N] bool, known_lattice
    [B] bool, atom_types [N] (1..100), frac_coords [N,3], lattices [B,3,3]; table: `level_table`'s; z = `draws`' triple.  Returns the
    state in `dtype` with the known elements replaced and every other element a plain cast of the input."""
    a, x, l = (v.detach().cpu().to(dtype).clone() for v in state)
    l = l.view(-1, 3, 3)
    kt, kx, kl = (torch.as_tensor(m).bool() for m in (cond.known_types, cond.known_coords, cond.known_lattice))
    zl, zx, zt = (v.to(dtype) for v in z)
    onehot = torch.nn.functional.one_hot(cond.atom_types.long().clamp(1, NUM_TYPES) - 1, num_classes=NUM_TYPES).to(dtype)
    l0, x0 = cond.lattices.to(dtype).view(-1, 3, 3), cond.frac_coords.to(dtype)
    if level == 0:
        nl, nx, nt = l0, x0 % 1.0, onehot
    else:
        c0, c1, sig = table[level].to(dtype)
        nl = c0 * l0 + c1 * zl
        nx = (x0 + sig * zx) % 1.0
        nt = c0 * onehot + c1 * zt
    l[kl], x[kx], a[kt] = nl[kl], nx[kx], nt[kt]
    return a, x, l
