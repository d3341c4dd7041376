"""Reference arithmetic of the property predictor (include/matinvent_hip_scalar.h) in float32 and float64 on top of
oracle.diffcsp_oracle: the reference's CSPNet(pred_scalar=True) forward -- cspnet_forward's tap of the last layer, the final LayerNorm,
scatter_mean, the head -- the masked loss with its statistics and closed-form seeds, and gradients by autograd on the oracle's parameter
dict (with `decoder.scalar_out.weight` [P, H] and `decoder.scalar_out.bias` [P] in it).  Plain torch, CPU; a helper, not a test."""
import torch

from oracle import diffcsp_oracle as O

MSE, L1 = "mse", "l1"


def clean_inputs(atom_types, frac, lengths, angles, times, time_dim, dtype):
    """What the device builds from a labelled crystal: one-hot type rows, coordinates wrapped to [0, 1), the lattice matrix, the time embedding."""
    at = torch.as_tensor(atom_types).long()
    onehot = torch.nn.functional.one_hot(at - 1, num_classes=O.MAX_ATOMIC_NUM).to(dtype)
    fr = torch.as_tensor(frac).to(dtype) % 1.0
    lat = O.lattice_params_to_matrix(torch.as_tensor(lengths).to(dtype), torch.as_tensor(angles).to(dtype))
    t_emb = O.time_embedding(torch.as_tensor(times).long(), time_dim).to(dtype)
    return t_emb, onehot, fr, lat


def pooled(hf, num_atoms):
    na = torch.as_tensor(num_atoms).long()
    n2g = torch.repeat_interleave(torch.arange(len(na)), na)
    return O.scatter_mean(hf, n2g, len(na))


def head(gf, W, bias):
    return gf @ W.t() + bias


def forward(P, hp, t_emb, onehot, frac, lattices, num_atoms, dtype=torch.float32):
    """-> (out [B, P], gf [B, H], hf [N, H]) in `dtype`; P may hold tensors that require grad."""
    c = lambda v: v.to(dtype) if v.is_floating_point() else v
    na = torch.as_tensor(num_atoms).long()
    n2g = torch.repeat_interleave(torch.arange(len(na)), na)
    taps = {}
    Pc = {k: c(v) for k, v in P.items()}
    O.cspnet_forward(Pc, hp, c(t_emb), c(onehot), c(frac), c(lattices), na, n2g, taps=taps)
    h = taps[f"h_{hp.num_layers - 1}"]
    if hp.ln:
        h = O._layer_norm(h, Pc["decoder.final_layer_norm.weight"], Pc["decoder.final_layer_norm.bias"])
    gf = O.scatter_mean(h, n2g, len(na))
    return head(gf, Pc["decoder.scalar_out.weight"], Pc["decoder.scalar_out.bias"]), gf, h


def loss(out, yhat, have, count_global, kind=MSE):
    """The stated loss as tensor ops (differentiable in `out`): sum_p (1 / P) sum_{b: have} l(e_bp) / count_global[p]; a property with
    count_global = 0 contributes nothing.  A missing target's yhat is never used (it may hold anything, NaN included)."""
    dt = out.dtype
    hv = torch.as_tensor(have).bool()
    cg = torch.as_tensor(count_global).to(dt)
    e = torch.where(hv, out - torch.where(hv, torch.as_tensor(yhat).to(dt), torch.zeros((), dtype=dt)), torch.zeros((), dtype=dt))
    l = e * e if kind == MSE else e.abs()
    per = l.sum(dim=0)
    Pn = out.shape[1]
    ok = cg > 0
    return (torch.where(ok, per / torch.where(ok, cg, torch.ones_like(cg)), torch.zeros_like(per)) / Pn).sum()


def stats(out, yhat, have, count_global, kind=MSE):
    """[1 + 3 P]: the loss, then per property sum e^2, sum |e|, present targets (this batch's)."""
    dt = out.dtype
    hv = torch.as_tensor(have).bool()
    e = torch.where(hv, out - torch.where(hv, torch.as_tensor(yhat).to(dt), torch.zeros((), dtype=dt)), torch.zeros((), dtype=dt))
    per = torch.stack([(e * e).sum(dim=0), e.abs().sum(dim=0), hv.to(dt).sum(dim=0)], dim=1).reshape(-1)
    return torch.cat([loss(out, yhat, have, count_global, kind).reshape(1), per])


def seeds(out, yhat, have, count_global, kind=MSE, accum=1):
    """d (loss / accum) / d out in closed form: 2 e / (P count accum) or sign(e) / (P count accum) where the target is present, else 0."""
    dt = out.dtype
    hv = torch.as_tensor(have).bool()
    cg = torch.as_tensor(count_global).to(dt)
    e = torch.where(hv, out - torch.where(hv, torch.as_tensor(yhat).to(dt), torch.zeros((), dtype=dt)), torch.zeros((), dtype=dt))
    num = 2 * e if kind == MSE else torch.sign(e)
    den = out.shape[1] * torch.where(cg > 0, cg, torch.ones_like(cg)) * accum
    return torch.where(hv, num / den, torch.zeros((), dtype=dt))


def seeds_autograd(out, yhat, have, count_global, kind=MSE, accum=1):
    o = out.detach().clone().requires_grad_(True)
    (loss(o, yhat, have, count_global, kind) / accum).backward()
    return o.grad


def micro_step(P, hp, t_emb, onehot, frac, lattices, num_atoms, yhat, have, count_global, kind=MSE, accum=1, dtype=torch.float32):
    """The whole micro-step by autograd: dict(out, gf, stats [1 + 3 P], d_out, grads = {name: d (loss / accum) / d P[name]}), a tensor the
    loss does not reach (the three diffusion heads) with a zero gradient."""
    c = lambda v: v.to(dtype) if v.is_floating_point() else v
    Pg = {k: c(v).detach().clone().requires_grad_(True) for k, v in P.items()}
    out, gf, _ = forward(Pg, hp, t_emb, onehot, frac, lattices, num_atoms, dtype)
    out.retain_grad()
    total = loss(out, yhat, have, count_global, kind) / accum
    names = list(Pg)
    gs = torch.autograd.grad(total, [Pg[k] for k in names] + [out], allow_unused=True)
    grads = {k: (torch.zeros_like(Pg[k]) if g is None else g) for k, g in zip(names, gs[:-1])}
    return dict(out=out.detach(), gf=gf.detach(), stats=stats(out.detach(), yhat, have, count_global, kind), d_out=gs[-1], grads=grads)


def subset(fs, idx):
    """The crystals `idx` of a set dict(num_atoms, atom_types, frac, lengths, angles), in that order."""
    na = torch.as_tensor(fs["num_atoms"]).long()
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(na, 0)])
    rows = torch.cat([torch.arange(int(off[i]), int(off[i + 1])) for i in idx])
    i = torch.as_tensor(idx).long()
    return dict(num_atoms=na[i], lengths=fs["lengths"][i], angles=fs["angles"][i], frac=fs["frac"][rows], atom_types=fs["atom_types"][rows])


def build_set(num_atoms, seed):
    """A labelled-crystal set: lengths in 4..10, angles in 70..110 degrees, coordinates in [0, 1), atomic numbers 1..94."""
    g = torch.Generator().manual_seed(seed)
    na = torch.as_tensor(num_atoms).long()
    B, N = len(na), int(na.sum())
    return dict(num_atoms=na, lengths=4.0 + 6.0 * torch.rand(B, 3, generator=g), angles=70.0 + 40.0 * torch.rand(B, 3, generator=g),
                frac=torch.rand(N, 3, generator=g), atom_types=torch.randint(1, 95, (N,), generator=g))
