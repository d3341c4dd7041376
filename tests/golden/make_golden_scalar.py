#!/usr/bin/env python
"""Generate g15_pred_scalar.npz by running the reference's own CSPNet(pred_scalar=True, smooth=True, ...).

Runs only where the reference tree is present (see make_golden.py: the reference modules are imported through tests/oracle_shims).
Output (committed): tests/golden/g15_pred_scalar.npz -- data only: the clean inputs of three crystals of [1, 7, 3] atoms, the state
dict of the tiny configuration g5a uses (H = 64, L = 2, F = 8, LayerNorm) and the network's output [3, 1].
Usage: python tests/golden/make_golden_scalar.py
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests", "oracle_shims"))
sys.path.insert(0, "/root/reference")
_pf = types.ModuleType("pipeline.filters")
_pf.invalid_filter = None
_pk = types.ModuleType("pipeline")
_pk.filters = _pf
_pk.__path__ = []
sys.modules["pipeline"] = _pk
sys.modules["pipeline.filters"] = _pf

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(8)

from models.diffcsp import cspnet as ref_cspnet  # noqa: E402
from models.diffcsp import diffusion as ref_diffusion  # noqa: E402
from models.diffcsp import utils as ref_utils  # noqa: E402

NUM_ATOMS = [1, 7, 3]


def main():
    torch.manual_seed(15)
    net = ref_cspnet.CSPNet(hidden_dim=64, num_layers=2, max_atoms=100, num_freqs=8, edge_style="fc", ln=True, ip=True, cutoff=7.0,
                            max_neighbors=20, latent_dim=256, pred_type=True, smooth=True, pred_scalar=True)
    g = torch.Generator().manual_seed(150)
    na = torch.tensor(NUM_ATOMS, dtype=torch.long)
    B, N = len(NUM_ATOMS), int(na.sum())
    n2g = torch.repeat_interleave(torch.arange(B), na)
    lengths = 4.0 + 6.0 * torch.rand(B, 3, generator=g)
    angles = 70.0 + 40.0 * torch.rand(B, 3, generator=g)
    frac = torch.rand(N, 3, generator=g)
    types = torch.randint(1, 95, (N,), generator=g)
    times = torch.zeros(B, dtype=torch.long)
    t_emb = ref_diffusion.SinusoidalTimeEmbeddings(256)(times)
    lattices = ref_utils.lattice_params_to_matrix_torch(lengths, angles)
    onehot = torch.nn.functional.one_hot(types - 1, num_classes=100).float()
    with torch.no_grad():
        out = net(t_emb, onehot, frac, lattices, na, n2g)
    assert tuple(out.shape) == (B, 1)
    arrs = dict(num_atoms=na, atom_types=types, frac=frac, lengths=lengths, angles=angles, times=times, t_emb=t_emb, lattices=lattices,
                onehot=onehot, scalar=out)
    arrs.update({"P__decoder." + k: v for k, v in net.state_dict().items()})
    path = os.path.join(HERE, "g15_pred_scalar.npz")
    np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in arrs.items()})
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB, {len(arrs)} arrays)")


if __name__ == "__main__":
    main()
