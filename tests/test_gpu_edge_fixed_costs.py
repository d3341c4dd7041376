"""The register-tile edge GEMMs after their fixed costs were cut (csrc/edge_stage.hip, csrc/loop_waits.h): the self-edge
workgroups of the first edge GEMM (first in the grid, one thread per 8-column chunk, 16-byte plane stores) and every k-loop length at
which the loops' fill and drain take another unrolled form, against the plane GEMM bit for bit and against the oracle."""
import ctypes as C

import pytest
import torch

from oracle import diffcsp_oracle as O
from tests.gpu_util import load_decoder

pytestmark = pytest.mark.gpu

RAGGED = [1, 7, 20, 3, 2]   # 33 nodes: not a multiple of the 8 nodes of a self-edge workgroup; a one-atom crystal (a self edge and no pair); a pair tile across crystals


def _inputs(num_atoms, seed):
    g = torch.Generator().manual_seed(seed)
    B, N = len(num_atoms), sum(num_atoms)
    t_emb = O.time_embedding(torch.full((B,), 77), 256).cuda()
    at, fr = torch.randn(N, 100, generator=g).cuda(), torch.rand(N, 3, generator=g).cuda()
    lat = (5 * torch.eye(3) + 0.5 * torch.randn(B, 3, 3, generator=g)).cuda()
    seeds = [torch.randn(B, 3, 3, generator=g).cuda(), torch.randn(N, 3, generator=g).cuda(), torch.randn(N, 100, generator=g).cuda()]
    return t_emb, at, fr, lat, seeds


@pytest.mark.parametrize("num_atoms", [RAGGED, [2]], ids=["ragged-33-nodes", "one-pair-row"])
@pytest.mark.parametrize("F", [8, 16, 32, 40, 128])
def test_first_edge_gemm_register_tile_form_vs_plane_gemm_bit_identical(F, num_atoms):
    """H = 128, L = 2, num_freqs 8 / 16 / 32 / 40 / 128: K = 64, 128, 192, 256, 768, i.e. 2, 4, 6, 8 and 24 k-tiles -- the three short
    forms of the k-loop, the shortest general one (fill and drain back to back) and the benchmark's.  The forced register-tile form
    against the plane GEMM: the three outputs and every layer's node features of the inference forward, and the outputs and the whole
    parameter gradient of the training forward (the backward pass reads every pre-activation the forward put on the tape, the self
    edges' included), must be equal bit for bit."""
    from matinvent_amd import _lib
    from matinvent_amd.cspnet import CSPNet
    lib = _lib.load()
    H, L = 128, 2
    hp = O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F)
    P = O.init_params(hp, seed=21)
    net = CSPNet(hidden_dim=H, num_layers=L, num_freqs=F, latent_dim=256, ln=True, smooth=True, pred_type=True, device="cuda")
    load_decoder(net, P)
    t_emb, at, fr, lat, seeds = _inputs(num_atoms, 23 + F)
    bt = net.make_batch(num_atoms)
    res = {}
    try:
        for form in (1, 0):
            lib.mi_debug_set_edge1_fused(form)
            with torch.no_grad():
                outs = [x.clone() for x in net(t_emb, at, fr, lat, None, batch=bt)]
            outs += [net.tap(bt, l + 1).clone() for l in range(L)]
            net.theta.grad = None
            with torch.enable_grad():
                touts = net(t_emb, at, fr, lat, None, batch=bt)
                sum((o * s).sum() for o, s in zip(touts, seeds)).backward()
            torch.cuda.synchronize()
            res[form] = outs + [x.detach().clone() for x in touts] + [net.theta.grad.clone()]
    finally:
        lib.mi_debug_set_edge1_fused(9)
    names = ["pred_l", "pred_x", "pred_t"] + [f"h after layer {l}" for l in range(L)] + ["train pred_l", "train pred_x", "train pred_t", "grad theta"]
    for a, b, w in zip(res[1], res[0], names):
        assert torch.isfinite(a).all(), w
        assert torch.equal(a, b), f"{w}: register-tile form differs from the plane GEMM, max abs diff {float((a - b).abs().max()):.3e}"


@pytest.mark.parametrize("K", [64, 128, 192, 512])
def test_gemm_rt_short_and_long_k_loops_bit_identical(K):
    """gemm_rt at M = 130 (a ragged second row tile), N = 256 and 2, 4, 6 and 16 k-tiles against the 128 x 128 plane kernel."""
    from matinvent_amd import _lib
    lib = _lib.load()
    if lib.mi_plane_format() != 2:
        pytest.skip("the register-tile kernel exists in the fp16 two-plane build")
    M, N = 130, 256
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).cuda()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).cuda()
    outs = []
    try:
        _lib.check(lib.mi_debug_set_planes_big(0, 1))
        for rt, rows in ((2, 1), (0, 0)):
            _lib.check(lib.mi_debug_set_planes_rt(rt, rows))
            for _ in range(3 if rt else 1):   # (repeated: an under-counted wait would show as run-to-run differences)
                out = torch.full((M, N), float("nan"), device="cuda")
                _lib.check(lib.mi_debug_gemm(2, C.c_void_p(A.data_ptr()), K, C.c_void_p(W.data_ptr()), K, C.c_void_p(out.data_ptr()), N, M, N, K, None))
                torch.cuda.synchronize()
                outs.append(out)
    finally:
        _lib.check(lib.mi_debug_set_planes_rt(2, 16384))
        _lib.check(lib.mi_debug_set_planes_big(1, 65536))
    for o in outs[:-1]:
        assert torch.equal(o, outs[-1])
    ref = A.double() @ W.double().t()
    assert (outs[0].double() - ref).abs().max().item() / ref.abs().max().item() < 3e-6   # (the plane format's bound in tests/test_gpu_gemm.py)


def test_second_edge_gemm_register_tile_form_vs_oracle():
    """H = 512, L = 1, F = 8 on the ragged batch with the second edge GEMM forced onto the register-tile kernel, against the oracle forward at
    the forward tests' tolerance (the two device forms group M2's partial sums differently: they are not bit-equal to each other)."""
    from matinvent_amd import _lib
    from matinvent_amd.cspnet import CSPNet
    lib = _lib.load()
    H, L, F = 512, 1, 8
    hp = O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F)
    P = O.init_params(hp, seed=21)
    net = CSPNet(hidden_dim=H, num_layers=L, num_freqs=F, latent_dim=256, ln=True, smooth=True, pred_type=True, device="cuda")
    load_decoder(net, P)
    t_emb, at, fr, lat, _ = _inputs(RAGGED, 29)
    bt = net.make_batch(RAGGED)
    try:
        lib.mi_debug_set_edge2_fused(1)
        with torch.no_grad():
            outs = [x.cpu() for x in net(t_emb, at, fr, lat, None, batch=bt)]
    finally:
        lib.mi_debug_set_edge2_fused(1)   # (the default)
    na = torch.tensor(RAGGED)
    n2g = torch.repeat_interleave(torch.arange(len(RAGGED)), na)
    with torch.no_grad():
        ref = O.cspnet_forward(P, hp, t_emb.cpu(), at.cpu(), fr.cpu(), lat.cpu(), na, n2g)
    for a, b, w in zip(outs, ref, ["pred_l", "pred_x", "pred_t"]):
        scale = max(1.0, float(b.abs().max()))
        err = float((a - b).abs().max())
        assert err <= 3e-5 * scale, f"{w}: max abs err {err:.3e} > 3e-5 * {scale:.3g}"
