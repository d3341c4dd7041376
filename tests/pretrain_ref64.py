"""Float64 reference of the supervised training micro-step's own arithmetic (matinvent_amd/csrc/pretrain.hip: pretrain_time_kernel,
pretrain_loss_kernel, pretrain_stats_kernel; include/matinvent_hip_pretrain.h states the formulas) with no network and no device code in
it, built on tests/ft_ref64.py (the forward noising, the fine-tune sets): torch's F.mse_loss over ALL elements of the mini-batch, its
derivatives with respect to the predictions (the seeds of the network backward), the per-crystal sums of squares and the four statistics.
Every function takes the predictions as an argument, so a test that knows them exactly (zero head weights) holds a yardstick without
network error.

Also here: oracle_training_step, the reference's training_step (diffusion.py:457-486: add_noise, the network, three F.mse_loss, the
cost-weighted sum) through oracle.diffcsp_oracle on the CPU in a chosen precision (float64: what pins this file; float32: the yardstick
of the device's tolerance), oracle_fit, the literal epoch loop around it with oracle.adam_step, and evaluate_ref, the weighting of
pretrain.evaluate over mini-batches.  Plain torch, CPU; shared by the CPU and the GPU tests."""
import torch

from oracle import diffcsp_oracle as O
from tests import ft_ref64 as R

NUM_TYPES = R.NUM_TYPES
COSTS = R.COSTS
STATS = ("loss", "loss_lattice", "loss_coord", "loss_type")


def parts(preds, targets, num_atoms, dtype=torch.float64):
    """[B, 3]: crystal b's sums of (pred - target)^2 over its 9 lattice, 3 n_b coordinate and 100 n_b type elements."""
    na, n2g = R._batch(num_atoms)
    (pl, px, pt), (rl, tx, rt) = ([v.to(dtype) for v in g] for g in (preds, targets))
    per = lambda v: torch.zeros(len(na), dtype=dtype).index_add(0, n2g, v.sum(dim=-1))
    return torch.stack([((pl - rl) ** 2).sum(dim=(-1, -2)), per((px - tx) ** 2), per((pt - rt) ** 2)], dim=1)


def stats(preds, targets, costs, b_global, n_global, dtype=torch.float64):
    """[4] = (loss, loss_lattice, loss_coord, loss_type): F.mse_loss of a mini-batch of b_global crystals / n_global atoms of which
    these are the rows held here (the whole mini-batch: b_global = B, n_global = N, and the three are torch's means)."""
    (pl, px, pt), (rl, tx, rt) = ([v.to(dtype) for v in g] for g in (preds, targets))
    ll = ((pl - rl) ** 2).sum() / (9 * b_global)
    lx = ((px - tx) ** 2).sum() / (3 * n_global)
    lt = ((pt - rt) ** 2).sum() / (NUM_TYPES * n_global)
    return torch.stack([costs[0] * ll + costs[1] * lx + costs[2] * lt, ll, lx, lt])


def seeds(preds, targets, costs, b_global, n_global, accum):
    """d (loss / accum) / d (pl, px, pt) in closed form (float64)."""
    (pl, px, pt), (rl, tx, rt) = ([v.double() for v in g] for g in (preds, targets))
    return (2 * costs[0] * (pl - rl) / (9 * b_global * accum), 2 * costs[1] * (px - tx) / (3 * n_global * accum),
            2 * costs[2] * (pt - rt) / (NUM_TYPES * n_global * accum))


def elementwise(preds, targets, costs, num_atoms, b_global, n_global, accum):
    """The same four statistics, per-crystal sums and seeds one element at a time in Python floats (float64), with no tensor op in it:
    what pins `stats`, `parts` and `seeds`.  Returns (stats [4], parts [B][3], (seed_l, seed_x, seed_t) as nested lists)."""
    na = [int(v) for v in num_atoms]
    (pl, px, pt), (rl, tx, rt) = ([v.double().reshape(v.shape[0], -1).tolist() for v in g] for g in (preds, targets))
    P, sl, sx, st, row = [], [], [], [], 0
    for b, n in enumerate(na):
        q = [0.0, 0.0, 0.0]
        sl.append([])
        for k in range(9):
            e = pl[b][k] - rl[b][k]
            q[0] += e * e
            sl[-1].append(2 * costs[0] * e / (9 * b_global * accum))
        for i in range(row, row + n):
            sx.append([])
            st.append([])
            for k in range(3):
                e = px[i][k] - tx[i][k]
                q[1] += e * e
                sx[-1].append(2 * costs[1] * e / (3 * n_global * accum))
            for k in range(NUM_TYPES):
                e = pt[i][k] - rt[i][k]
                q[2] += e * e
                st[-1].append(2 * costs[2] * e / (NUM_TYPES * n_global * accum))
        row += n
        P.append(q)
    ll = sum(q[0] for q in P) / (9 * b_global)
    lx = sum(q[1] for q in P) / (3 * n_global)
    lt = sum(q[2] for q in P) / (NUM_TYPES * n_global)
    return [costs[0] * ll + costs[1] * lx + costs[2] * lt, ll, lx, lt], P, (sl, sx, st)


def evaluate_ref(preds, targets, costs, num_atoms, batch_size, dtype=torch.float64):
    """pretrain.evaluate's weighting: the set cut into mini-batches of `batch_size` crystals in order, every mini-batch's `stats` taken
    with the counts of the WHOLE set, summed -- the set's four losses whatever batch_size is."""
    na, _ = R._batch(num_atoms)
    B, N = len(na), int(na.sum())
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(na, 0)]).tolist()
    total = torch.zeros(4, dtype=dtype)
    for lo in range(0, B, batch_size):
        hi = min(B, lo + batch_size)
        rows = lambda g: (g[0][lo:hi], g[1][off[lo]:off[hi]], g[2][off[lo]:off[hi]])
        total = total + stats(rows(preds), rows(targets), costs, B, N, dtype)
    return total


# ---- the oracle on the same inputs --------------------------------------------------------------------------------------------------

def oracle_training_step(hp, P, tables, fs, nz, dtype, times, costs=COSTS, b_global=None, n_global=None, accum=1, freqs=None, grad=False):
    """DiffCSPModule.training_step as the reference states it, through oracle.diffcsp_oracle on the CPU with every floating-point input
    (the set, the schedule tables, the noise, the parameters P, the time embedding's frequency table) taken to `dtype` first:
    add_noise at the per-crystal `times`, cspnet_forward, three mse over all elements (sum / count, with the counts of the whole
    mini-batch when these crystals are a shard of it), total = loss / accum.  Returns dict(targets, preds, t_emb, stats [4], parts
    [B,3], grads = {name: d total / d P[name]} with grad=True)."""
    c = lambda v: v.to(dtype) if v.is_floating_point() else v
    noised = R.oracle_add_noise(tables, fs, nz, dtype, None, times)
    B, N = len(fs["num_atoms"]), int(torch.as_tensor(fs["num_atoms"]).sum())
    b_global, n_global = B if b_global is None else b_global, N if n_global is None else n_global
    t = torch.as_tensor(times).long()
    t_emb = c(noised[0][0]) if freqs is None else R.time_embedding(t, c(freqs))
    Pg = {k: c(v).detach().clone().requires_grad_(grad) for k, v in P.items()}
    preds = O.cspnet_forward(Pg, hp, t_emb, *noised[0][1:])
    rand_l, tar_x, rand_t = noised[1]
    sq = lambda p, q: torch.nn.functional.mse_loss(p, q, reduction="sum")
    ll, lx, lt = sq(preds[0], rand_l) / (9 * b_global), sq(preds[1], tar_x) / (3 * n_global), sq(preds[2], rand_t) / (NUM_TYPES * n_global)
    loss = costs[0] * ll + costs[1] * lx + costs[2] * lt
    out = dict(targets=noised[1], preds=tuple(v.detach() for v in preds), t_emb=t_emb, stats=torch.stack([loss, ll, lx, lt]).detach(),
               parts=parts(tuple(v.detach() for v in preds), noised[1], fs["num_atoms"], dtype))
    if grad:
        names = list(Pg)
        out["grads"] = dict(zip(names, torch.autograd.grad(loss / accum, [Pg[k] for k in names], allow_unused=True)))
    return out


def subset(fs, idx):
    """The crystals `idx` of a set (ft_ref64.SET_KEYS), in that order."""
    na = torch.as_tensor(fs["num_atoms"]).long()
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(na, 0)])
    rows = torch.cat([torch.arange(int(off[i]), int(off[i + 1])) for i in idx]) if len(idx) else torch.zeros(0, dtype=torch.long)
    i = torch.as_tensor(idx).long()
    return dict(num_atoms=na[i], lengths=fs["lengths"][i], angles=fs["angles"][i], frac_coords=fs["frac_coords"][rows], atom_types=fs["atom_types"][rows])


def oracle_fit(hp, P0, tables, fs, plan_fn, times_fn, noise_fn, epochs, lr, accum=1, costs=COSTS, freqs=None, dtype=torch.float32):
    """The literal training loop: for every epoch the mini-batches plan_fn(epoch) (index lists into the set `fs`), each one
    oracle_training_step at times_fn(epoch, step, B) with the noise noise_fn(epoch, step), gradients accumulated over `accum`
    mini-batches, oracle.adam_step (one state for the whole run) at the end of every window and behind the last mini-batch.  Returns
    (the trained parameters, the per-epoch means of the four statistics [epochs][4])."""
    A = {k: v.detach().clone().to(dtype) for k, v in P0.items()}
    state, logged = {}, []
    for epoch in range(epochs):
        plan = plan_fn(epoch)
        grads = {k: torch.zeros_like(v) for k, v in A.items()}
        acc = torch.zeros(4, dtype=dtype)
        for step, idx in enumerate(plan):
            o = oracle_training_step(hp, A, tables, subset(fs, idx), noise_fn(epoch, step), dtype, times_fn(epoch, step, len(idx)), costs,
                                     accum=accum, freqs=freqs, grad=True)
            acc = acc + o["stats"]
            for k, g in o["grads"].items():
                grads[k] += g
            if (step + 1) % accum == 0 or step + 1 == len(plan):
                with torch.no_grad():
                    O.adam_step(A, grads, state, lr)
                for g in grads.values():
                    g.zero_()
        logged.append((acc / len(plan)).tolist())
    return A, logged
