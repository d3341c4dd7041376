"""Autograd bridge: CSPNet forward/backward through the C ABI as ONE differentiable op.

The reference's fine-tune step calls `.backward()` on a scalar built with ordinary tensor ops
on the network's three outputs (pipeline/mat_invent.py:158-164).  Keeping that surface means the
network has to be a differentiable op returning ordinary tensors: forward =
mi_cspnet_forward_train (keeps its activations inside the batch handle), backward =
mi_cspnet_backward (hand-written kernels; gradient w.r.t. the flat parameter vector only).
"""
import torch

from . import _lib
from .cspnet import MAX_ATOMIC_NUM, _ptr, _stream


class CSPNetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, net, batch, t_emb, atom_types, frac, lattices):
        lib = _lib.load()
        net.sync()
        dev = theta.device
        B, N = batch.num_graphs, batch.num_nodes
        lat_out = torch.empty(B, 3, 3, device=dev)
        coord_out = torch.empty(N, 3, device=dev)
        type_out = torch.empty(N, MAX_ATOMIC_NUM, device=dev)
        _lib.check(lib.mi_cspnet_forward_train(net._h, batch._h, _ptr(t_emb), _ptr(atom_types), _ptr(frac), _ptr(lattices),
                                               _ptr(lat_out), _ptr(coord_out), _ptr(type_out), _stream()), "mi_cspnet_forward_train")
        ctx.net, ctx.batch = net, batch
        ctx.nparams = theta.numel()
        return lat_out, coord_out, type_out

    @staticmethod
    def backward(ctx, d_lat, d_coord, d_type):
        lib = _lib.load()
        net, batch = ctx.net, ctx.batch
        dev = net.theta.device
        B, N = batch.num_graphs, batch.num_nodes
        z = lambda g, *s: (torch.zeros(*s, device=dev) if g is None else g.contiguous().float())
        d_lat, d_coord, d_type = z(d_lat, B, 3, 3), z(d_coord, N, 3), z(d_type, N, MAX_ATOMIC_NUM)
        grad = torch.zeros(ctx.nparams, device=dev)
        _lib.check(lib.mi_cspnet_backward(net._h, batch._h, _ptr(d_lat), _ptr(d_coord), _ptr(d_type), _ptr(grad), _stream()),
                   "mi_cspnet_backward")
        return grad, None, None, None, None, None, None


class TrajLogProbFunction(torch.autograd.Function):
    """DiffCSPModule.forward_logprb (diffusion.py:158-227) as ONE differentiable op: forward = mi_traj_logprob with its tapes kept (two
    training evaluations on the handle pair `batches`, then the log-probability kernel), backward = mi_traj_logprob_backward (the seed
    kernel, then the hand-written backward on both tapes).  Returns log_prob_l, log_prob_t, log_prob_x [B] and the corrector's
    predictions (lattice [B,3,3], coordinates [N,3], types [N,100]), all differentiable with respect to theta.  `pair`: the module's
    handle pair (diffcsp._TrajPair); a later call on it makes this call's backward raise."""

    @staticmethod
    def forward(ctx, theta, net, pair, times, coef, T, freqs, atom_types, frac, frac_mid, lattices, next_types, next_frac, next_lat):
        lib = _lib.load()
        net.sync()
        b_corr, b_pred = pair.handles
        dev = theta.device
        B, N = b_corr.num_graphs, b_corr.num_nodes
        lp = torch.empty(3, B, device=dev)
        pl, px, pt = torch.empty(B, 3, 3, device=dev), torch.empty(N, 3, device=dev), torch.empty(N, MAX_ATOMIC_NUM, device=dev)
        _lib.check(lib.mi_traj_logprob(net._h, b_corr._h, b_pred._h, _ptr(times), _ptr(coef), T, _ptr(freqs), _ptr(atom_types), _ptr(frac),
                                       _ptr(frac_mid), _ptr(lattices), _ptr(next_types), _ptr(next_frac), _ptr(next_lat), _ptr(lp), _ptr(pl),
                                       _ptr(px), _ptr(pt), 1, _stream()), "mi_traj_logprob")
        ctx.net, ctx.pair, ctx.call = net, pair, pair.calls
        ctx.nparams = theta.numel()
        return lp[0], lp[1], lp[2], pl, px, pt

    @staticmethod
    def backward(ctx, g_l, g_t, g_x, d_pl, d_px, d_pt):
        lib = _lib.load()
        net, (b_corr, b_pred) = ctx.net, ctx.pair.handles
        if ctx.pair.calls != ctx.call:
            raise _lib.MIError(_lib.MI_ESTATE, "forward_logprb backward: a later forward_logprb call with the same atom counts overwrote this "
                                               "call's tapes (one pending backward per atom-count vector)")
        dev = net.theta.device
        B = b_corr.num_graphs
        g = torch.stack([torch.zeros(B, device=dev) if v is None else v.float() for v in (g_l, g_t, g_x)]).contiguous()
        c = lambda v: None if v is None else v.contiguous().float()
        d_pl, d_px, d_pt = c(d_pl), c(d_px), c(d_pt)
        grad = torch.zeros(ctx.nparams, device=dev)
        _lib.check(lib.mi_traj_logprob_backward(net._h, b_corr._h, b_pred._h, _ptr(g), _ptr(d_pl), _ptr(d_px), _ptr(d_pt), _ptr(grad),
                                                _stream()), "mi_traj_logprob_backward")
        return (grad,) + (None,) * 13
