"""Fixed costs inside a workgroup of the two edge GEMMs (edge_gemm1b_kernel, edge_gemm2b_kernel: csrc/edge_stage.hip) at the headline
shape, from the kernels' phase clocks: prologue to the first barrier, the k-loop up to its last three iterations, the last three
iterations, the epilogue -- and the life of a self-edge workgroup of the first GEMM.  One forward alone on the chip (no second chain),
the last layer's launch.  (profiles/edge_gemm_fixed_costs.md holds the readings; scripts/edge2_phases.py has the occupancy view.)
usage (GPU box): python scripts/edge_fixed_costs.py [crystals]"""
import ctypes as C
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from matinvent_amd import _lib  # noqa: E402
from matinvent_amd.cspnet import CSPNet  # noqa: E402
from oracle import diffcsp_oracle as O  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
n, H, L, F = 20, 512, 6, 128
lib = _lib.load()
torch.manual_seed(0)
net = CSPNet(hidden_dim=H, num_layers=L, num_freqs=F, latent_dim=256, ln=True, smooth=True, pred_type=True, device="cuda")
g = torch.Generator().manual_seed(1)
N = B * n
t_emb = O.time_embedding(torch.full((B,), 500), 256).cuda()
at, fr = torch.randn(N, 100, generator=g).cuda(), torch.rand(N, 3, generator=g).cuda()
lat = (4 * torch.eye(3) + torch.randn(B, 3, 3, generator=g)).cuda()
bt = net.make_batch([n] * B)
torch.set_grad_enabled(False)
for _ in range(3):
    net(t_emb, at, fr, lat, None, batch=bt)


def phases(name, c):
    """c: [workgroups][8] -- stamps 0 entry, 1 first barrier, 2 end of the loop, 3 exit, 6 head of the third iteration from the end"""
    c = c[(c[:, 3] > 0) & (c[:, 6] > 0)]
    if len(c) == 0:
        print(f"{name}: no workgroup stamped (another kernel form ran)")
        return
    cols = [("prologue to first barrier", c[:, 1] - c[:, 0]), ("loop up to the last three iterations", c[:, 6] - c[:, 1]),
            ("last three iterations", c[:, 2] - c[:, 6]), ("epilogue", c[:, 3] - c[:, 2]), ("workgroup life", c[:, 3] - c[:, 0])]
    print(f"{name}: {len(c)} workgroups; s_memtime ticks, median / mean / max")
    for nm, d in cols:
        print(f"  {nm:38s} {np.median(d):9.0f} {d.mean():9.1f} {d.max():9d}")


reps = 5
for rep in range(reps):
    nt2 = (B * n * n + 127) // 128 * 2
    clk2 = torch.zeros(nt2 * 8, dtype=torch.int64, device="cuda")
    lib.mi_debug_edge2_clock(C.c_void_p(clk2.data_ptr()))
    net(t_emb, at, fr, lat, None, batch=bt)
    torch.cuda.synchronize()
    lib.mi_debug_edge2_clock(None)
    npairs = B * n * (n - 1) // 2
    nt1 = ((npairs + 127) // 128 + 7) // 8 * 8 * (H // 128)
    clk1 = torch.zeros(nt1 * 8, dtype=torch.int64, device="cuda")
    lib.mi_debug_edge1_clock(C.c_void_p(clk1.data_ptr()))
    net(t_emb, at, fr, lat, None, batch=bt)
    torch.cuda.synchronize()
    lib.mi_debug_edge1_clock(None)
    print(f"--- reading {rep + 1} of {reps}, {B} crystals")
    phases("edge_gemm2b", clk2.cpu().numpy().reshape(nt2, 8))
    c1 = clk1.cpu().numpy().reshape(nt1, 8)
    phases("edge_gemm1b pair tiles", c1)
    # self-edge workgroup d stamps its entry and exit into slots 4 / 5 of row d (s_memtime is not one clock for the whole chip: only the
    # differences inside a workgroup are read here, none between workgroups)
    sd = c1[(c1[:, 4] > 0) & (c1[:, 5] > 0)]
    if len(sd):
        life = sd[:, 5] - sd[:, 4]
        print(f"edge_gemm1b self-edge workgroups: {len(sd)}; life median / mean / max {np.median(life):.0f} {life.mean():.1f} {life.max()} ticks")
