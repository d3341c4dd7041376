"""Float64 restatement of the resampling jumps (matinvent_amd/csrc/resample.hip: resample_jump_kernel) with no device code in
it: the forward process between two noise levels a and b = a + j

    l = c0 l + c1 z        a = c0 a + c1 z        x = (x + s z) mod 1
    c0 = sqrt(abar_b / abar_a)   c1 = sqrt(1 - abar_b / abar_a)   s = sqrt(sigma_b^2 - sigma_a^2)

applied to EVERY element of a state, the jump table [T + 1][3] built from dict(alphas_cumprod, sigmas) in float64, and the draws of the
noise contract: oracle.diffcsp_oracle's numpy Philox with the draw ids 24 / 25 / 26, the step field = the level jumped TO and the element
index (node_offset + atom) * width + column (graph_offset + crystal for the lattice).  RePaint's published schedule (get_schedule_jump)
is restated here too, with level = their index + 1.  Plain torch / numpy on the CPU; shared by the CPU and the GPU tests.
`jump(..., dtype=torch.float32)` is the same formulas separately rounded in float32: the yardstick of the device's tolerance."""
import torch

from oracle import diffcsp_oracle as O

NUM_TYPES = 100
DRAW_JUMP_L, DRAW_JUMP_X, DRAW_JUMP_T, DRAW_VISIT = 24, 25, 26, 27


def draws(seed, to_level, num_atoms, node_offset=0, graph_offset=0):
    """(z_l [B,3,3], z_x [N,3], z_t [N,100]) float32: the contract's normals of one jump TO `to_level` for a batch that starts at global
    atom `node_offset`, global crystal `graph_offset`."""
    na = torch.as_tensor(num_atoms).long()
    B, N = len(na), int(na.sum())
    f = lambda draw, n, off, *shape: torch.from_numpy(O.philox_normal(int(seed), int(to_level), draw, n, off).copy()).view(*shape)
    return (f(DRAW_JUMP_L, B * 9, graph_offset * 9, B, 3, 3), f(DRAW_JUMP_X, N * 3, node_offset * 3, N, 3),
            f(DRAW_JUMP_T, N * NUM_TYPES, node_offset * NUM_TYPES, N, NUM_TYPES))


def jump_table(tables, j):
    """[T + 1, 3] float64 = (c0, c1, s) of a -> a + j from dict(alphas_cumprod, sigmas) taken to float64 first; rows past T - j zero."""
    ac, sig = tables["alphas_cumprod"].double(), tables["sigmas"].double()
    n = len(ac)
    tab = torch.zeros(n, 3, dtype=torch.float64)
    for a in range(n - j):
        ratio = ac[a + j] / ac[a]
        tab[a, 0] = torch.sqrt(ratio)
        tab[a, 1] = torch.sqrt(torch.clamp(1.0 - ratio, min=0.0))
        tab[a, 2] = torch.sqrt(torch.clamp(sig[a + j] ** 2 - sig[a] ** 2, min=0.0))
    return tab


def jump(state, table, from_level, z, dtype=torch.float64):
    """state = (atom_types [N,100], frac [N,3], lattices [B,3,3]); table: `jump_table`'s (any dtype); z = `draws`' triple at the level
    jumped to.  Returns the jumped state in `dtype`, every operation rounded there."""
    a, x, l = (v.detach().cpu().to(dtype) for v in state)
    zl, zx, zt = (v.to(dtype) for v in z)
    c0, c1, s = table[from_level].to(dtype)
    x = (x + s * zx) % 1.0
    return c0 * a + c1 * zt, x % 1.0, c0 * l.view(-1, 3, 3) + c1 * zl


def repaint_levels(t_T, jump_length, jump_n_sample):
    """RePaint's get_schedule_jump (Lugmayr et al. 2022, their sampling schedule) with level = their index + 1, a forward jump being their
    `jump_length` single forward steps: the visited levels with every single forward step listed."""
    jumps = {i: jump_n_sample - 1 for i in range(0, t_T - jump_length, jump_length)}
    t, ts = t_T, []
    while t >= 1:
        t -= 1
        ts.append(t)
        if jumps.get(t, 0) > 0:
            jumps[t] -= 1
            for _ in range(jump_length):
                t += 1
                ts.append(t)
    ts.append(-1)
    return [v + 1 for v in ts]


def expand(levels, j):
    """A schedule whose forward jumps are one move of j levels -> the same with each jump as j single forward steps (RePaint's listing)."""
    out = [levels[0]]
    for a, b in zip(levels[:-1], levels[1:]):
        out += [b] if b == a - 1 else list(range(a + 1, b + 1))
        assert b == a - 1 or b == a + j, (a, b)
    return out
